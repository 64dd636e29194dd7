"""GPU: the masked mode (true per-crop lengths in attention, InstanceNorm and WBCE). The property
under test: masked mode on a padded batch computes, for every crop, what the existing code
computes on that crop alone, unpadded — real-row outputs, the loss and every parameter gradient;
padded rows of every output and gradient are exactly 0 and nothing in the padding is ever used."""
import functools

import numpy as np
import pytest
import torch

from oracle import dpfm_model_oracle as M

pytestmark = pytest.mark.gpu

NAN = float("nan")
D, H = 16, 2
ATT_N, ATT_M = 200, 600
# full length; a single key (key blocks 1, 2 empty: dk = 0 in truth); one past a 256-key block and a
# 128-query block; exactly one tile with the forward's second query block wholly padded
ATT_QLEN, ATT_KLEN = [200, 1, 129, 64], [600, 1, 257, 64]


def _att_inputs(qlen, klen, N=ATT_N, M_=ATT_M, seed=5, pad=0.0):
    """q, k, v, go with `pad` in every padded position."""
    g = torch.Generator().manual_seed(seed)
    B = len(qlen)
    q = torch.randn(B, D, H, N, generator=g) * 2
    k = torch.randn(B, D, H, M_, generator=g) * 2
    v = torch.randn(B, D, H, M_, generator=g)
    go = torch.randn(B, D, H, N, generator=g)
    for b in range(B):
        q[b, :, :, qlen[b]:] = pad
        go[b, :, :, qlen[b]:] = pad
        k[b, :, :, klen[b]:] = pad
        v[b, :, :, klen[b]:] = pad
    return q, k, v, go


def _att_ref(q, k, v):
    """modeling/dpfm.py:29-37 (test_model_gpu.test_attention_fwd_bwd's formula)."""
    scores = torch.einsum("bdhn,bdhm->bhnm", q, k) / D ** 0.5
    return torch.einsum("bhnm,bdhm->bdhn", torch.nn.functional.softmax(scores, dim=-1), v)


def _i32(x, device):
    return torch.tensor(x, dtype=torch.int32, device=device)


def _run_masked(q, k, v, go, qlen, klen, device):
    from dpfm_amd import ops
    ins = [x.to(device).requires_grad_() for x in (q, k, v)]
    out = ops.attention(*ins, qlen=_i32(qlen, device), klen=_i32(klen, device))
    out.backward(go.to(device))
    return [t.detach().cpu() for t in (out, *(x.grad for x in ins))]


def test_attention_per_crop_truth(device):
    """Masked attention on the padded batch vs the formula on each crop's slices alone: real rows
    of out, dq, dk, dv within 3x the fp32 CPU reference's own error + 1e-6 (1 + scale) of the fp64
    truth (test_attention_fwd_bwd's bar), and bit-equal — forward AND backward — to the existing
    ops.attention called on the contiguous slices of that crop alone: the tile sequences are the
    same, and the dQ scale 0.25 is exact wherever it is applied (in the kernel for one key block,
    in the reduce launch otherwise), so the backward does not legitimately differ either."""
    from dpfm_amd import ops
    q, k, v, go = _att_inputs(ATT_QLEN, ATT_KLEN)
    mine = _run_masked(q, k, v, go, ATT_QLEN, ATT_KLEN, device)
    for b, (nq, nk) in enumerate(zip(ATT_QLEN, ATT_KLEN)):
        sl = [q[b:b + 1, :, :, :nq], k[b:b + 1, :, :, :nk], v[b:b + 1, :, :, :nk]]
        gs = go[b:b + 1, :, :, :nq]
        res = []
        for dt, dev in ((torch.float64, "cpu"), (torch.float32, "cpu"), (torch.float32, device)):
            ins = [x.detach().clone().contiguous().to(device=dev, dtype=dt).requires_grad_() for x in sl]
            out = (ops.attention if dev == device else _att_ref)(*ins)
            (out * gs.contiguous().to(device=dev, dtype=dt)).sum().backward()
            res.append([t.detach().cpu() for t in (out, *(x.grad for x in ins))])
        got = [mine[0][b:b + 1, :, :, :nq], mine[1][b:b + 1, :, :, :nq], mine[2][b:b + 1, :, :, :nk],
               mine[3][b:b + 1, :, :, :nk]]
        scale = max(t.abs().max().item() for t in res[0])
        for name, t, r, alone, d in zip(["out", "dq", "dk", "dv"], *res, got):
            e_ref = (r.double() - t).abs().max().item()
            e_mine = (d.double() - t).abs().max().item()
            print(f"crop {b} {name}: e_mine {e_mine:.3e} e_ref {e_ref:.3e} scale {scale:.3e}")
            assert e_mine <= 3 * e_ref + 1e-6 * (1 + scale), (b, name, e_mine, e_ref)
            assert torch.equal(d, alone), (b, name, (d - alone).abs().max().item())


def test_attention_padding_never_used_and_zero(device):
    """Zeros vs NaN in every padded position of q, k, v, go, with out, lse, dq, dk, dv and the work
    buffer pre-filled with NaN (raw entry points): real rows bit-identical, padded rows of out, dq,
    dk, dv exactly 0, lse (0, 0) there, no NaN anywhere; a crop without keys and one without
    queries give all-zero finite outputs and gradients."""
    from dpfm_amd import _lib, ops
    qlen, klen = ATT_QLEN + [200, 0], ATT_KLEN + [0, 600]
    B, N, M_ = len(qlen), ATT_N, ATT_M
    P = _lib.ptr
    ql, kl = _i32(qlen, device), _i32(klen, device)
    runs = []
    for pad in (0.0, NAN):
        q, k, v, go = (t.to(device) for t in _att_inputs(qlen, klen, pad=pad))
        out, dq = torch.full_like(q, NAN), torch.full_like(q, NAN)
        dk, dv = torch.full_like(k, NAN), torch.full_like(v, NAN)
        lse = torch.full((B, H, N, 2), NAN, device=device)
        work = ops.attention_bwd_work(B, D, H, N, M_, device)
        work.fill_(NAN)
        s = _lib.stream(device)
        _lib.call("pk_attention_fwd_varlen", P(q), P(k), P(v), B, D, H, N, M_, 0, 0, P(ql), P(kl), P(out), P(lse), s)
        _lib.call("pk_attention_bwd_varlen", P(q), P(k), P(v), P(out), P(go), P(lse), B, D, H, N, M_, 0, 0, P(ql),
                  P(kl), P(work), P(dq), P(dk), P(dv), 0, 0, s)
        runs.append([t.cpu() for t in (out, dq, dk, dv, lse)])
    for name, a, b_ in zip(["out", "dq", "dk", "dv", "lse"], *runs):
        assert not torch.isnan(a).any() and not torch.isnan(b_).any(), name
        assert torch.equal(a, b_), name
    out, dq, dk, dv, lse = runs[1]
    for b in range(B):
        nq, nk = (qlen[b], klen[b]) if klen[b] > 0 and qlen[b] > 0 else (0, 0)  # an empty side: all zero
        assert (out[b, :, :, nq:] == 0).all() and (dq[b, :, :, nq:] == 0).all(), b
        assert (lse[b, :, nq:] == 0).all(), b
        assert (dk[b, :, :, nk:] == 0).all() and (dv[b, :, :, nk:] == 0).all(), b
    assert out[0].abs().max() > 0 and dq[2].abs().max() > 0 and dk[2].abs().max() > 0  # (not vacuous)


@pytest.mark.parametrize("N,M_", [(ATT_N, ATT_M), (77, 130)])
def test_attention_full_lengths_equal_unmasked(device, N, M_):
    """qlen = N, klen = M for every crop: bit-equal to the unmasked op, forward and backward
    (three key blocks, and one: the in-kernel dQ scale of the unmasked single-block path)."""
    from dpfm_amd import ops
    B = 3
    q, k, v, go = _att_inputs([N] * B, [M_] * B, N=N, M_=M_, seed=N)
    mine = _run_masked(q, k, v, go, [N] * B, [M_] * B, device)
    ins = [x.to(device).requires_grad_() for x in (q, k, v)]
    out = ops.attention(*ins)
    out.backward(go.to(device))
    for name, a, b_ in zip(["out", "dq", "dk", "dv"], mine, (out, *(x.grad for x in ins))):
        assert torch.equal(a, b_.detach().cpu()), name


def _norm_truth(x, dy, lens, eps=1e-5):
    """fp64 from the formula: mean and biased variance over the first n points; 0 past them."""
    y, dx = torch.zeros_like(x, dtype=torch.float64), torch.zeros_like(x, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        xr = x[b, :, :n].double().requires_grad_()
        mean = xr.mean(1, keepdim=True)
        var = (xr - mean).square().mean(1, keepdim=True)
        yr = torch.relu((xr - mean) / torch.sqrt(var + eps))
        yr.backward(dy[b, :, :n].double())
        y[b, :, :n], dx[b, :, :n] = yr.detach(), xr.grad
    return y, dx


@pytest.mark.parametrize("B,C,N,lens", [(3, 8, 300, [300, 2, 65]), (2, 4, 2100, [2100, 2049])])
def test_instnorm_masked(device, B, C, N, lens):
    """Masked InstanceNorm + ReLU vs the formula in fp64 (1e-5 of scale, test_instnorm_relu_fwd_bwd's
    bar); register-tile and streaming paths; y and dx exactly 0 past n; NaN in the padding of x and
    dy changes nothing."""
    from dpfm_amd import ops
    g = torch.Generator().manual_seed(B * C + N)
    x = torch.randn(B, C, N, generator=g) * 3 + 1
    dy = torch.randn(B, C, N, generator=g)
    yt, dxt = _norm_truth(x, dy, lens)
    res = []
    for pad in (None, NAN):
        xp, dyp = x.clone(), dy.clone()
        if pad is not None:
            for b, n in enumerate(lens):
                xp[b, :, n:] = pad
                dyp[b, :, n:] = pad
        xd = xp.to(device).requires_grad_(True)
        yd = ops.instnorm_relu(xd, 1e-5, lens=_i32(lens, device))
        yd.backward(dyp.to(device))
        res.append((yd.detach().cpu(), xd.grad.cpu()))
    (y, dx), (y2, dx2) = res
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    e_y, e_dx = (y.double() - yt).abs().max().item(), (dx.double() - dxt).abs().max().item()
    print(f"instnorm N={N}: e_y {e_y:.3e} / {yt.abs().max().item():.3e}  e_dx {e_dx:.3e} / {dxt.abs().max().item():.3e}")
    assert e_y <= 1e-5 * yt.abs().max().item()
    assert e_dx <= 1e-5 * dxt.abs().max().item()
    for b, n in enumerate(lens):
        assert (y[b, :, n:] == 0).all() and (dx[b, :, n:] == 0).all(), b


@pytest.mark.parametrize("N", [300, 2100])
def test_instnorm_masked_one_and_no_point(device, N):
    """lens = 1 and lens = 0 rows: all-zero outputs, finite statistics (mean = the point / 0, invstd
    = 1 / sqrt(eps)), with NaN in the padding and in the pre-filled outputs."""
    from dpfm_amd import _lib
    B, C, eps = 2, 8, 1e-5
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, C, N, generator=g)
    first = x[0, :, 0].clone()
    x[0, :, 1:] = NAN
    x[1] = NAN
    x = x.to(device)
    dy = torch.full((B, C, N), NAN, device=device)
    dy[0, :, 0] = 1.0
    y, dx = torch.full_like(x, NAN), torch.full_like(x, NAN)
    mean, invstd = torch.full((B * C,), NAN, device=device), torch.full((B * C,), NAN, device=device)
    lens = _i32([1, 0], device)
    P, s = _lib.ptr, _lib.stream(device)
    _lib.call("pk_instnorm_relu_fwd_varlen", P(x), B * C, N, eps, P(y), P(mean), P(invstd), C, P(lens), s)
    _lib.call("pk_instnorm_relu_bwd_varlen", P(x), P(dy), P(mean), P(invstd), B * C, N, P(dx), C, P(lens), s)
    assert (y == 0).all() and (dx == 0).all()
    mean, invstd = mean.cpu(), invstd.cpu()
    assert torch.isfinite(mean).all() and torch.isfinite(invstd).all()
    assert torch.equal(mean[:C], first) and (mean[C:] == 0).all()
    torch.testing.assert_close(invstd, torch.full((B * C,), 1.0 / np.sqrt(np.float32(eps)), dtype=torch.float32),
                               rtol=1e-6, atol=0)


def _wbce_inputs():
    g = torch.Generator().manual_seed(21)
    B, N1, N2 = 3, 300, 70
    n1, n2 = [300, 1, 129], [1, 70, 33]
    p12 = torch.rand(B, N1, generator=g) * 0.98 + 0.01
    p21 = torch.rand(B, N2, generator=g) * 0.98 + 0.01
    t12 = (torch.rand(B, N1, generator=g) < 0.3).float()
    t21 = (torch.rand(B, N2, generator=g) < 0.6).float()
    for b in range(B):  # padding the masked op must not see
        p12[b, n1[b]:], t12[b, n1[b]:] = 2.0, 1.0
        p21[b, n2[b]:], t21[b, n2[b]:] = 2.0, 1.0
    return p12, p21, t12, t21, n1, n2


def _wbce_truth(p, t, n, dt):
    """The oracle's weighted_bce on each crop's slice: (loss [B], dloss_b / dp [B, N] with 0 past n)."""
    loss, grad = [], torch.zeros(p.shape, dtype=dt)
    for b in range(p.shape[0]):
        pr = p[b, :n[b]].to(dt).requires_grad_()
        l = M.weighted_bce(pr, t[b, :n[b]].to(dt))
        l.backward()
        loss.append(l.detach())
        grad[b, :n[b]] = pr.grad
    return torch.stack(loss), grad


def test_wbce_masked(device):
    """pk_wbce_varlen vs the oracle's weighted_bce on the slices in fp64: loss and gradients within
    3x the fp32 CPU error of the same formula + 1e-6 of scale; gradients exactly 0 past n (the
    padding holds p = 2, t = 1, which the unmasked formula could not even evaluate)."""
    from dpfm_amd import ops
    p12, p21, t12, t21, n1, n2 = _wbce_inputs()
    pd = [p.to(device).requires_grad_() for p in (p12, p21)]
    loss = ops.weighted_bce_pair(pd[0], pd[1], t12.to(device), t21.to(device), n1=_i32(n1, device), n2=_i32(n2, device))
    loss.sum().backward()
    for which, (p, t, n) in enumerate(((p12, t12, n1), (p21, t21, n2))):
        lt, gt = _wbce_truth(p, t, n, torch.float64)
        lr, gr = _wbce_truth(p, t, n, torch.float32)
        lm, gm = loss[which].detach().cpu().double(), pd[which].grad.cpu().double()
        for name, tt, rr, mm in (("loss", lt, lr, lm), ("grad", gt, gr, gm)):
            e_ref, e_mine = (rr.double() - tt).abs().max().item(), (mm - tt).abs().max().item()
            print(f"wbce {which} {name}: e_mine {e_mine:.3e} e_ref {e_ref:.3e} scale {tt.abs().max().item():.3e}")
            assert e_mine <= 3 * e_ref + 1e-6 * tt.abs().max().item(), (which, name, e_mine, e_ref)
        for b in range(p.shape[0]):
            assert (gm[b, n[b]:] == 0).all(), (which, b)


def test_wbce_empty_crop(device):
    """n = 0: loss 0, gradient 0, finite."""
    from dpfm_amd import ops
    p12, p21, t12, t21, _, _ = _wbce_inputs()
    pd = [p.to(device).requires_grad_() for p in (p12, p21)]
    loss = ops.weighted_bce_pair(pd[0], pd[1], t12.to(device), t21.to(device), n1=_i32([0, 0, 40], device),
                                 n2=_i32([0, 40, 0], device))
    loss.sum().backward()
    l = loss.detach().cpu()
    assert torch.isfinite(l).all() and (l[0, :2] == 0).all() and l[1, 0] == 0 and l[1, 2] == 0
    assert l[0, 2] > 0 and l[1, 1] > 0  # (the non-empty crops: 40 real points each)
    assert (pd[0].grad[:2] == 0).all() and (pd[1].grad[0] == 0).all() and (pd[1].grad[2] == 0).all()
    assert torch.isfinite(pd[0].grad).all() and torch.isfinite(pd[1].grad).all()


def test_dpfm_loss_masked(device):
    """DPFMLoss.forward_batched(..., n1, n2): acc_loss is the per-crop sum of the oracle's
    weighted_bce over the slices (x w_acc / B; bar as in test_wbce_masked); fmap_loss and nce_loss
    are bit-equal to the unmasked call, since they do not see the flag."""
    from dpfm_amd.utils.loss import DPFMLoss, nce_select
    p12, p21, t12, t21, n1, n2 = _wbce_inputs()
    B, N1, N2 = p12.shape[0], p12.shape[1], p21.shape[1]
    g = torch.Generator().manual_seed(3)
    C12, C_gt = torch.randn(B, 30, 30, generator=g) * 0.1, torch.randn(B, 30, 30, generator=g) * 0.1
    f1, f2 = torch.randn(B, N1, 32, generator=g), torch.randn(B, N2, 32, generator=g)
    cap = 16
    pairs = torch.zeros(B, cap, 2, dtype=torch.int64)  # real pair indices only, inside both true lengths
    pairs[0, :, 1] = 0
    pairs[0, :, 0] = torch.arange(cap)
    pairs[1, :, 0] = 0
    pairs[1, :, 1] = torch.arange(cap)
    pairs[2, :, 0], pairs[2, :, 1] = torch.arange(cap), torch.arange(cap)
    npairs = torch.tensor([cap, cap, cap], dtype=torch.int64)
    crit = DPFMLoss(w_fmap=1, w_acc=0.7, w_nce=1, nce_t=0.07, nce_num_pairs=8)
    dev = lambda t: t.to(device)  # noqa: E731
    sel = nce_select(dev(npairs), cap, 8, None)
    # the unmasked call cannot take p = 2 in its padding: give it in-range padding (its acc_loss is
    # not compared; fmap and nce do not read o12 / o21)
    args = [dev(C12), dev(C_gt), dev(pairs), dev(npairs), dev(f1), dev(f2)]
    _, log_u = crit.forward_batched(*args, dev(p12.clamp(max=0.5)), dev(p21.clamp(max=0.5)), dev(t12), dev(t21),
                                    selection=sel)
    _, log_m = crit.forward_batched(*args, dev(p12), dev(p21), dev(t12), dev(t21), selection=sel,
                                    n1=_i32(n1, device), n2=_i32(n2, device))
    assert torch.equal(log_u["fmap_loss"], log_m["fmap_loss"]) and torch.equal(log_u["nce_loss"], log_m["nce_loss"])
    acc = {}
    for dt in (torch.float64, torch.float32):
        l12, _ = _wbce_truth(p12, t12, n1, dt)
        l21, _ = _wbce_truth(p21, t21, n2, dt)
        acc[dt] = float(((l12 + l21) * 0.7 / B).sum())
    e_ref, e_mine = abs(acc[torch.float32] - acc[torch.float64]), abs(float(log_m["acc_loss"]) - acc[torch.float64])
    print(f"acc_loss: e_mine {e_mine:.3e} e_ref {e_ref:.3e} value {acc[torch.float64]:.6f}")
    assert e_mine <= 3 * e_ref + 1e-6 * abs(acc[torch.float64])
    _, log_c = crit.forward_batched_composed(*args, dev(p12), dev(p21), dev(t12), dev(t21), selection=sel,
                                             n1=_i32(n1, device), n2=_i32(n2, device))
    assert abs(float(log_c["acc_loss"]) - acc[torch.float64]) <= 3 * e_ref + 1e-6 * abs(acc[torch.float64])


# ------------------------------------------------------------------------------ the model property

MODEL_N1, MODEL_N2 = [256, 130, 65], [200, 64, 129]
KEYS = ("xyz", "mass", "evals", "evecs")
OUT_NAMES = ["C", "o12", "o21", "f1", "f2"]


def _loss_a(o):  # model_parity's "overlap+features" on whatever rows `o` holds
    return o[1].sum() + o[2].sum() + o[3].square().sum() + o[4].square().sum()


def _loss_b(o):  # model_parity's "fmap"
    return o[0].sum()


def _real_rows(o, b, n1, n2):
    """Crop b's (C, o12, o21, f1, f2) restricted to its real rows, from a batched output."""
    o12, o21 = (o[1], o[2]) if o[1].dim() == 2 else (o[1][None], o[2][None])
    return [o[0][b], o12[b, :n1], o21[b, :n2], o[3][b, :n1], o[4][b, :n2]]


def _model_items(seed=0):
    from dpfm_amd.pipeline import lbo_padded
    rng = np.random.default_rng(seed)
    items = []
    for b, (a, c) in enumerate(zip(MODEL_N1, MODEL_N2)):
        cm, ce, cv = lbo_padded(a, 2 * (seed + b))
        pm, pe, pv = lbo_padded(c, 2 * (seed + b) + 1)
        x1 = (rng.normal(size=(a, 3)) * 6 + 100).astype(np.float32)
        x2 = (rng.normal(size=(c, 3)) * 6 + 100).astype(np.float32)
        items.append(({"xyz": x1, "mass": cm, "evals": ce, "evecs": cv},
                      {"xyz": x2, "mass": pm, "evals": pe, "evecs": pv}, {"obj_id": 0}))
    return items


def _grads(model):
    return [torch.zeros(p.shape, dtype=torch.float64) if p.grad is None else p.grad.detach().cpu().double()
            for p in model.parameters()]


def _per_crop(model, batch, dev, dt):
    """`model` on each crop alone, unpadded (B = 1): real-row outputs per crop and, for the two
    losses, every parameter's gradient summed over the crops."""
    outs, grads = [], []
    for b, (a, c) in enumerate(zip(MODEL_N1, MODEL_N2)):
        one = {k: {kk: v[kk][b:b + 1, :(a if k == "shape1" else c)].to(device=dev, dtype=dt) if kk != "evals"
                   else v[kk][b:b + 1].to(device=dev, dtype=dt) for kk in KEYS} for k, v in batch.items()}
        with torch.no_grad():
            outs.append([t.detach().cpu().double() for t in _real_rows(model(one), 0, a, c)])
    for fn in (_loss_a, _loss_b):
        model.zero_grad()
        for b, (a, c) in enumerate(zip(MODEL_N1, MODEL_N2)):
            one = {k: {kk: v[kk][b:b + 1, :(a if k == "shape1" else c)].to(device=dev, dtype=dt) if kk != "evals"
                       else v[kk][b:b + 1].to(device=dev, dtype=dt) for kk in KEYS} for k, v in batch.items()}
            fn(_real_rows(model(one), 0, a, c)).backward()  # .grad accumulates over the crops
        grads.append(_grads(model))
    return outs, grads


@functools.lru_cache(maxsize=None)
def _model_reference(device_str):
    """Computed once for both parametrisations: the padded batch (collate(counts=True)), the shared
    weights, the fp64 per-crop truth and the two yardsticks (the oracle in fp32 on the CPU, the
    existing unmasked HIP DPFMNet on each crop alone)."""
    from dpfm_amd.dataset.helpers import collate
    from dpfm_amd.models.dpfm import DPFMNet
    device = torch.device(device_str)
    CAD, PC, _ = collate(_model_items(), counts=True)
    batch = {"shape1": CAD, "shape2": PC}
    assert CAD["xyz"].shape[1] == 256 and PC["xyz"].shape[1] == 200
    assert CAD["n"].tolist() == MODEL_N1 and PC["n"].tolist() == MODEL_N2
    torch.manual_seed(7)
    ref = M.DPFMNet()
    with torch.no_grad():
        ref.feature_extractor.block_0.diffusion.diffusion_time.uniform_(-0.001, 12)
        ref.feature_extractor.block_1.diffusion.diffusion_time.uniform_(-0.001, 12)
    truth = M.DPFMNet().double()
    truth.load_state_dict(ref.state_dict())
    alone = DPFMNet().to(device)
    alone.load_state_dict(ref.state_dict(), strict=True)
    t = _per_crop(truth, batch, "cpu", torch.float64)
    r = _per_crop(ref, batch, "cpu", torch.float32)
    g = _per_crop(alone, batch, device, torch.float32)
    return batch, ref.state_dict(), alone, t, r, g


def _err_out(outs, truth, i):
    return max((o[i] - t[i]).abs().max().item() for o, t in zip(outs, truth))


@pytest.mark.parametrize("fused", [True, False])
def test_masked_model_equals_per_crop(device, monkeypatch, fused):
    """DPFMNet(masked=True) on the ragged padded batch vs the fp64 oracle on each crop alone,
    unpadded: C and the real rows of o12, o21, f1, f2 within 3x the larger yardstick error + 1e-6
    (1 + |t|max); for model_parity's two losses on the real rows, every parameter's gradient within
    3x the larger yardstick error + 1e-6 x the global gradient norm. Both the fused node and the
    module path (FUSED_ATTN_PROP = False). Positive control: the unmasked model on the same padded
    batch misses that bar in o21 of the crop with the shortest shape 2."""
    from dpfm_amd.modeling import dpfm as modeling
    from dpfm_amd.models.dpfm import DPFMNet
    batch, state, alone, (t_out, t_gr), (r_out, r_gr), (g_out, g_gr) = _model_reference(str(device))
    monkeypatch.setattr(modeling, "FUSED_ATTN_PROP", fused)
    mine = DPFMNet(masked=True).to(device)
    mine.load_state_dict(state, strict=True)
    dbatch = {k: {kk: v[kk].to(device) for kk in KEYS + ("n",)} for k, v in batch.items()}
    rows = lambda o: [_real_rows(o, b, a, c) for b, (a, c) in enumerate(zip(MODEL_N1, MODEL_N2))]  # noqa: E731
    with torch.no_grad():
        m_out = [[t.detach().cpu().double() for t in r] for r in rows(mine(dbatch))]
    bars = {}
    for i, name in enumerate(OUT_NAMES):
        e = [_err_out(o, t_out, i) for o in (r_out, g_out, m_out)]
        tmax = max(t[i].abs().max().item() for t in t_out)
        bars[name] = 3 * max(e[0], e[1]) + 1e-6 * (1 + tmax)
        print(f"{name}: e_cpu32 {e[0]:.3e} e_alone {e[1]:.3e} e_masked {e[2]:.3e} bar {bars[name]:.3e}")
        assert e[2] <= bars[name], (name, e)
    for fi, (fn, label) in enumerate(((_loss_a, "overlap+features"), (_loss_b, "fmap"))):
        mine.zero_grad()
        sum(fn(r) for r in rows(mine(dbatch))).backward()
        m_gr = _grads(mine)
        floor = 1e-6 * torch.cat([g.reshape(-1) for g in t_gr[fi]]).norm().item()
        for i, (name, _) in enumerate(mine.named_parameters()):
            t = t_gr[fi][i]
            e = [(g[i] - t).norm().item() for g in (r_gr[fi], g_gr[fi], m_gr)]
            assert e[2] <= 3 * max(e[0], e[1]) + floor, (label, name, e, floor, t.norm().item())
    # positive control: unmasked, the padding reaches crop 1's 64 real shape-2 points
    with torch.no_grad():
        u21 = _real_rows(alone({k: {kk: v[kk] for kk in KEYS} for k, v in dbatch.items()}), 1, MODEL_N1[1],
                         MODEL_N2[1])[2].cpu().double()
    leak = (u21 - t_out[1][2]).abs().max().item()
    print(f"positive control: unmasked o21 of crop 1 differs by {leak:.3e} (bar {bars['o21']:.3e})")
    assert leak > bars["o21"], (leak, bars["o21"])


def test_masked_flags_must_agree(device):
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import InferStep, TrainStep
    with pytest.raises(ValueError):
        TrainStep(DPFMNet().to(device), masked=True)
    with pytest.raises(ValueError):
        InferStep(DPFMNet(masked=True).to(device))


def test_graphed_masked_train_step_matches_eager(device):
    """GraphedTrainStep over TrainStep(masked=True): the replayed step's loss, IR, flat gradient
    and updated parameters are bit-equal to the eager masked step from the same state
    (test_graphed_train_step_matches_eager's criterion and shape). The lengths stay on the device:
    a host read of them would fail the capture."""
    from dpfm_amd.dataset.object import CropFormation
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import GraphedTrainStep, TrainStep, make_frame_batch
    F, N = 4, 512
    fb, op = make_frame_batch(F, N, N, seed=90, device=device)
    cf = CropFormation(n1=N, npoint=N, seed=1)
    torch.manual_seed(0)
    m_eager = DPFMNet(masked=True).to(device)
    m_graph = DPFMNet(masked=True).to(device)
    m_graph.load_state_dict(m_eager.state_dict())
    eager = TrainStep(m_eager, seed=5, capturable=True, masked=True)
    graph_step = TrainStep(m_graph, seed=5, capturable=True, masked=True)
    g = GraphedTrainStep(cf, graph_step, fb, op, warmup=2)
    for _ in range(2):
        eager(op, cf(fb))
    for _ in range(2):
        eager.load_state_from(graph_step)
        le = {k: v.clone() for k, v in eager(op, cf(fb)).items()}
        lg = {k: v.clone() for k, v in g().items()}
        torch.cuda.synchronize()
        for k in ("loss", "IR"):
            assert torch.equal(le[k], lg[k]), (k, le[k], lg[k])
        assert torch.isfinite(le["loss"]) and eager.flat.abs().max() > 0
        assert torch.equal(eager.flat, graph_step.flat)
        diff = [n for (n, a), b in zip(m_eager.named_parameters(), m_graph.parameters()) if not torch.equal(a, b)]
        assert not diff, diff
