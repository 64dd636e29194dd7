"""The scalar head of the DPFM loss node (csrc/loss_head.hip): pk_loss_head against fp64 with
distinct weights, crop counts that make a wave's crop loop iterate more than once and the clamp
mask at its inclusive bound; and the whole node (ops.dpfm_loss through DPFMLoss) with distinct
weights, a non-unit incoming gradient and enough gradient elements that pk_loss_scale strides."""
import pytest
import torch

from oracle import dpfm_model_oracle as M

pytestmark = pytest.mark.gpu

W = (0.7, 1.3, 0.1)  # w_fmap, w_acc, w_nce: all different, so that swapped weights show


def _head_inputs(B, K, seed):
    """C12, C_gt, nce [B], wb [2, B]. Even crops sit below FrobeniusLoss's clamp, odd crops above it
    (K >= 30). With K >= 30 the last crop has a squared error of exactly 1000 (ten entries differ
    by 10.0, the rest are equal) and, when there is one, its neighbour has 1100 (eleven entries)."""
    g = torch.Generator().manual_seed(seed)
    C = torch.round(torch.randn(B, K, K, generator=g) * 64) / 64  # multiples of 1/64: C + 10 is exact
    Cgt = C + 0.5 * torch.randn(B, K, K, generator=g)
    Cgt[1::2] = torch.randn(B, K, K, generator=g)[1::2] * 1.5
    edge = {}
    if K >= 30:
        for b, cnt in ((B - 1, 10), (B - 2, 11)):
            if b < 0:
                continue
            Cgt[b] = C[b]
            at = torch.randperm(K * K, generator=g)[:cnt]
            Cgt[b].view(-1)[at] += 10.0
            edge[b] = cnt
    nce = torch.rand(B, generator=g) * 8
    wb = torch.rand(2, B, generator=g)
    return C, Cgt, nce, wb, edge


@pytest.mark.parametrize("B", [1, 16, 17, 40])
@pytest.mark.parametrize("K", [1, 30, 32])
def test_loss_head_matches_fp64(device, K, B):
    """Each output within 1e-5 x the sum of the absolute values of its terms (the fp32 summation
    bound used for linear_wgrad). B = 17 and 40: wave w takes crops w, w + 16, w + 32. The crop at
    exactly 1000 passes its gradient (ATen's clamp backward is inclusive), the one at 1100 gets
    dC == 0."""
    from dpfm_amd import _lib
    C, Cgt, nce, wb, edge = _head_inputs(B, K, 31 * K + B)
    dev = [t.to(device) for t in (C, Cgt, nce, wb)]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=device)  # noqa: E731
    loss, logs, dC = nan(1), nan(3), nan(B, K, K)
    P = _lib.ptr
    _lib.call("pk_loss_head", P(dev[0]), P(dev[1]), B, K, P(dev[2]), P(dev[3]), W[0], W[1], W[2], P(loss), P(logs),
              P(dC), _lib.stream(device))
    loss, logs, dC = float(loss.cpu()), logs.cpu().double(), dC.cpu().double()
    d = C.double() - Cgt.double()
    f = (d ** 2).sum((1, 2))
    for b, cnt in edge.items():
        assert float(f[b]) == 100.0 * cnt  # exact in fp64 and in fp32, in any order
    fmap = torch.clamp(f, -1, 1000).mean() * W[0]
    nl = (nce.double() * W[2] / B).sum()
    al = ((wb[0].double() + wb[1].double()) * W[1] / B).sum()
    tol = 1e-5
    assert abs(float(logs[0]) - float(nl)) <= tol * float(nl.abs())
    assert abs(float(logs[1]) - float(al)) <= tol * float(al.abs())
    assert abs(float(logs[2]) - float(fmap)) <= tol * float(fmap.abs())
    assert abs(loss - float(fmap + al + nl)) <= tol * float(fmap + al + nl)  # every term is positive
    passes = (f >= -1) & (f <= 1000)
    ref = torch.where(passes[:, None, None], 2 * W[0] / B * d, torch.zeros_like(d))
    assert (dC - ref).abs().le(tol * ref.abs()).all(), float((dC - ref).abs().max())
    if K >= 30:
        assert bool(passes[B - 1]) and dC[B - 1].abs().sum() > 0 and int((dC[B - 1] != 0).sum()) == 10
        rest = passes[:max(B - 2, 0)]  # the other crops: even ones below the clamp, odd ones above it
        assert rest[::2].all() and not rest[1::2].any()
        if B >= 2:
            assert not bool(passes[B - 2]) and not dC[B - 2].any()


def test_loss_head_refuses_oversize(device):
    from dpfm_amd import _lib
    P = _lib.ptr
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
    for B, K in ((1025, 2), (2, 33), (0, 2)):
        n = max(B, 1)
        C, Cgt, nce, wb, dC, loss, logs = z(n, K, K), z(n, K, K), z(n), z(2, n), z(n, K, K), z(1), z(3)
        with pytest.raises(_lib.PoseKernError):
            _lib.call("pk_loss_head", P(C), P(Cgt), B, K, P(nce), P(wb), 1.0, 1.0, 1.0, P(loss), P(logs), P(dC),
                      _lib.stream(device))
    torch.cuda.synchronize(device)


def test_dpfm_loss_node_weights_and_scale_stride(device):
    """DPFMLoss(w_fmap=0.7, w_acc=1.3, w_nce=0.1) on B = 17 crops of 520 / 500 points, then
    (2.5 * loss).backward(): pk_loss_scale's range holds 17 x 1020 x 32 = 554 880 feature-gradient
    elements alone, above its 2048 x 256 = 524 288 threads, so it strides. Loss, the three logged
    terms and every input gradient against the oracle in fp64 (test_dpfm_loss_matches_oracle's
    tolerances: 1e-4 relative, 1e-4 of each gradient's scale). Again with only f2 and o12 requiring
    a gradient: the others stay None, those two are unchanged bit for bit."""
    from dpfm_amd import ops
    from dpfm_amd.utils.loss import DPFMLoss
    g = torch.Generator().manual_seed(17)
    B, N1, N2, K = 17, 520, 500, 30
    counts = [1500, 300, 512, 2000, 2, 511, 513, 40, 700, 512, 64, 1999, 17, 256, 257, 1000, 3]
    cap = max(counts)
    pairs = torch.zeros((B, cap, 2), dtype=torch.int64)
    for b, c in enumerate(counts):
        pairs[b, :c, 0] = torch.randint(0, N1, (c,), generator=g)
        pairs[b, :c, 1] = torch.randint(0, N2, (c,), generator=g)
    f1 = torch.randn(B, N1, 32, generator=g)
    f2 = torch.randn(B, N2, 32, generator=g)
    C = torch.randn(B, K, K, generator=g)
    C_gt = torch.randn(B, K, K, generator=g)
    C_gt[::2] = C[::2] + 0.5 * torch.randn(B, K, K, generator=g)[::2]  # even crops below the clamp
    o12 = torch.rand(B, N1, generator=g) * 0.98 + 0.01
    o21 = torch.rand(B, N2, generator=g) * 0.98 + 0.01
    g12 = (torch.rand(B, N1, generator=g) < 0.4).to(torch.int8)
    g21 = (torch.rand(B, N2, generator=g) < 0.6).to(torch.int8)
    npairs = torch.tensor(counts, dtype=torch.int64)
    ctr = torch.zeros(1, dtype=torch.int64, device=device)
    rows, valid = ops.nce_select(npairs.to(device), cap, 512, 9, ctr)
    sel = [rows[b][valid[b]].cpu() for b in range(B)]
    assert [len(s) for s in sel] == [min(c, 512) for c in counts]
    crit = DPFMLoss(w_fmap=W[0], w_acc=W[1], w_nce=W[2], nce_t=0.07, nce_num_pairs=512)
    names = ("C", "f1", "f2", "o12", "o21")

    def run(need):
        dv = [t.to(device).requires_grad_(n in need) for n, t in zip(names, (C, f1, f2, o12, o21))]
        loss, logs = crit.forward_batched(dv[0], C_gt.to(device), pairs.to(device), npairs.to(device), dv[1], dv[2],
                                          dv[3], dv[4], g12.to(device), g21.to(device), selection=(rows, valid))
        (2.5 * loss).backward()
        return loss, logs, dv

    loss, logs, dv = run(names)
    assert sum(t.numel() for t in dv) > 2048 * 256
    # oracle (fp64, CPU)
    rv = [t.double().requires_grad_(True) for t in (C, f1, f2, o12, o21)]
    plist = [pairs[b, :counts[b]] for b in range(B)]
    ref = M.dpfm_loss(rv[0], C_gt.double(), plist, sel, rv[1], rv[2], rv[3], rv[4], g12, g21, *W)
    (2.5 * ref).backward()
    assert abs(float(loss) - float(ref)) <= 1e-4 * abs(float(ref)), (float(loss), float(ref))
    with torch.no_grad():
        terms = {"fmap_loss": (W[0], 0.0, 0.0), "acc_loss": (0.0, W[1], 0.0), "nce_loss": (0.0, 0.0, W[2])}
        for key, w in terms.items():
            r = float(M.dpfm_loss(rv[0], C_gt.double(), plist, sel, rv[1], rv[2], rv[3], rv[4], g12, g21, *w))
            assert abs(float(logs[key]) - r) <= 1e-4 * abs(r), (key, float(logs[key]), r)
        assert float(logs["loss"]) == float(loss)
    assert rv[0].grad[::2].abs().max() > 0 and rv[0].grad[1::2].abs().max() == 0  # both clamp regimes
    for name, a, r in zip(names, dv, rv):
        ga, gr = a.grad.cpu().double(), r.grad
        scale = float(gr.abs().max())
        assert (ga - gr).abs().max().item() <= 1e-4 * scale + 1e-9, (name, (ga - gr).abs().max().item(), scale)
    # a subset of the inputs: the scale table holds two tensors, at other offsets
    loss2, _, dv2 = run(("f2", "o12"))
    assert float(loss2) == float(loss)
    assert dv2[0].grad is None and dv2[1].grad is None and dv2[4].grad is None
    assert torch.equal(dv2[2].grad, dv[2].grad) and torch.equal(dv2[3].grad, dv[3].grad)
