"""pk_nce_loss (csrc/nce.hip: row pass, column pass, scatter) against tests/_nce_ref.py at its slot
edges: ragged row groups, partner half 1 empty or partly filled, one-logit softmaxes, a valid mask
with holes, and padding.

Truth: _nce_ref.nce in fp64 with the difference-form distance. Yardstick: the same formulas in
fp32 on the CPU with the kernel's product-form distance. Per crop, for the loss, each side's
scale-free gradient in the Frobenius norm and each side's worst row:

    e_kernel <= 3 e_yardstick + 1e-5 scale

(3: this suite's convention; the floor: what the yardstick lacks, __expf on logits up to 2 / t = 29,
29 x 2^-23 = 3.5e-6 per term, taken about three times). Every test prints its largest
e_kernel / e_yardstick and e_kernel / bound.

No index in this file is out of range, and every device tensor a kernel reads is held by the
ops wrapper for the length of the call: nothing here can fault a kernel.
"""
import pytest
import torch

import _nce_ref as R

pytestmark = pytest.mark.gpu

T = R.T


def _pack(crops, S, cap, masks=None, seed=0):
    """pairs int64 [B, cap, 2], rows int64 [B, S], valid bool [B, S] that put crop b's pairs into
    the slots mask b allows (default: a prefix), in order, through distinct shuffled pair rows.
    Invalid slots point at pair rows no valid slot uses, which hold point 0 of both sides; when the
    pair buffer has no such row (cap == n) they point at row 0, as pk_nce_select's padding does."""
    g = torch.Generator().manual_seed(seed)
    B = len(crops)
    pairs = torch.zeros((B, cap, 2), dtype=torch.int64)
    rows = torch.zeros((B, S), dtype=torch.int64)
    valid = torch.zeros((B, S), dtype=torch.bool)
    for b, c in enumerate(crops):
        n = int(c["i1"].numel())
        m = masks[b] if masks is not None else torch.arange(S) < n
        assert int(m.sum()) == n and n <= cap
        perm = torch.randperm(cap, generator=g)
        valid[b] = m
        rows[b, m] = perm[:n]
        if cap > n:
            rows[b, ~m] = perm[n:][torch.arange(S - n) % (cap - n)]
        pairs[b, perm[:n], 0] = c["i1"]
        pairs[b, perm[:n], 1] = c["i2"]
    return pairs, rows, valid


def _stack(crops, key):
    return torch.stack([c[key] for c in crops])


def _run(device, crops, S, cap, **kw):
    from dpfm_amd import ops
    pairs, rows, valid = _pack(crops, S, cap, **kw)
    loss, g1, g2 = ops._nce_raw(_stack(crops, "f1").to(device), _stack(crops, "f2").to(device), pairs.to(device),
                                rows.to(device), valid.to(device).view(torch.uint8), T, True)
    return loss.cpu(), g1.cpu(), g2.cpu()


def _check(tag, crops, out):
    """Holds crop b of out = (loss [B], g1 [B, N1, 32], g2 [B, N2, 32]) to the bound; crops with at
    most one pair to exact zeros. Returns the largest e_kernel / bound."""
    worst_y, worst_b, missed = 0.0, 0.0, []
    for b, c in enumerate(crops):
        got = (out[0][b], out[1][b], out[2][b])
        assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all(), (tag, b)
        n = int(c["i1"].numel())
        if n <= 1:  # softmax over one logit: loss 0, zero gradients, exactly
            assert float(got[0]) == 0.0 and not got[1].any() and not got[2].any(), (tag, b, n)
            continue
        tr = R.nce(c["f1"], c["f2"], c["i1"], c["i2"])
        ya = R.nce(c["f1"], c["f2"], c["i1"], c["i2"], dtype=R.F32, mm=True)
        ek = R.errors(got, tr, c["f1"], c["f2"])
        ey = R.errors(ya, tr, c["f1"], c["f2"])
        for (name, e, s), (_, y, _) in zip(ek, ey):
            bound = 3 * y + 1e-5 * s
            worst_y = max(worst_y, e / y if y > 0 else 0.0)
            worst_b = max(worst_b, e / bound if bound > 0 else (0.0 if e == 0 else float("inf")))
            if not e <= bound:
                missed.append(f"crop {b} {name}: e_kernel {e:.3e} e_yardstick {y:.3e} scale {s:.3e}")
    print(f"nce {tag}: max e_kernel / e_yardstick = {worst_y:.2f}, max e_kernel / bound = {worst_b:.2f}")
    assert not missed, (tag, missed)
    return worst_b


@pytest.mark.parametrize("S", [1, 15, 16, 17, 63, 65, 200, 255, 256, 257, 300, 511])
def test_slot_edges(device, S):
    """Ragged last row groups (S not a multiple of 16), S below / at / past one block's 64 rows,
    partner half 1 all padding (S <= 256), partly filled (256 < S < 512), and the one-logit softmax.
    Four crops with S, about half of S, one and no valid slots; points repeat across slots (70 / 90
    points). Measured on MI355X, largest e_kernel / e_yardstick (and share of the bound) per S:
    15: 2.9 (0.07), 16: 2.0 (0.09), 17: 65 (0.06: the yardstick's own error is far below the floor
    there), 63: 1.0 (0.08), 65: 1.3 (0.07), 200: 1.6 (0.13), 255: 2.3 (0.14), 256: 1.5 (0.11),
    257: 1.7 (0.09), 300: 1.3 (0.08), 511: 1.3 (0.09); S = 1 is exact."""
    counts = [S, (S + 1) // 2, 1, 0]
    crops = [R.gaussian_crop(n, 70, 90, 1000 + 4 * S + b) for b, n in enumerate(counts)]
    out = _run(device, crops, S, S + 5, seed=S)
    _check(f"slots S={S}", crops, out)


def test_holes_in_valid(device):
    """valid is not a prefix: S = 300 with every third slot off equals the reference on the 200
    compacted slots (the kernel never assumes that valid slots come first). Measured on MI355X:
    e_kernel / e_yardstick 1.1, 0.10 of the bound."""
    S = 300
    mask = torch.arange(S) % 3 != 2
    crops = [R.gaussian_crop(200, 150, 170, 2000 + b) for b in range(2)]
    out = _run(device, crops, S, 400, masks=[mask, mask.roll(1)], seed=3)
    _check("holes", crops, out)


def test_padding_invariance(device):
    """The same 200 valid slots in an S = 200 buffer, in an S = 512 buffer, and with another pair
    capacity: padding adds exact zeros to every sum, in place. Asserted at the bound's floor
    (1e-5 of scale); whether the three agree bit for bit is printed. Measured on MI355X: bitwise."""
    crops = [R.gaussian_crop(200, 150, 170, 2100 + b) for b in range(2)]
    a = _run(device, crops, 200, 200, seed=4)
    b = _run(device, crops, 512, 200, seed=4)
    c = _run(device, crops, 512, 777, seed=5)
    _check("padding S=200", crops, a)
    bitwise = True
    for other in (b, c):
        for x, y in zip(a, other):
            bitwise = bitwise and torch.equal(x, y)
            assert (x.double() - y.double()).abs().max().item() <= 1e-5 * x.double().abs().max().item()
    print(f"nce padding invariance: bitwise = {bitwise}")
