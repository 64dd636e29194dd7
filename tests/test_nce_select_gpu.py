"""pk_nce_select against its integer-exact host model (tests/_nce_select_model.py, pinned by
test_nce_select_cpu.py): rows and valid bit for bit, the step counter's advance, the empty calls."""
import numpy as np
import pytest
import torch

import _nce_select_model as S

pytestmark = pytest.mark.gpu


def _counts(cap):
    return [0, 1, 2, 511, 512, 513, 1500, cap, cap + 7]


@pytest.mark.parametrize("ctr0", [0, 41])
@pytest.mark.parametrize("num,cap", [(8, 64), (8, 2000), (512, 64), (512, 2000)])
def test_select_matches_model(device, num, cap, ctr0):
    """Every count edge (none, one, two, around num, above it, cap and past cap), five crops per
    call so that the crop enters the key, k = min(num, cap) on both branches; two calls in a row:
    *ctr advances by exactly one per call and the second call draws with the advanced value."""
    from dpfm_amd import ops
    counts = _counts(cap)
    k = min(num, cap)
    for lo in range(0, len(counts), 5):
        cs = (counts[lo:lo + 5] + counts[:5])[:5]  # B = 5 (the second group is topped up from the first)
        ctr = torch.full((1,), ctr0, dtype=torch.int64, device=device)
        cd = torch.tensor(cs, dtype=torch.int64, device=device)
        for step in range(2):
            rows, valid = ops.nce_select(cd, cap, num, 9, ctr)
            assert rows.shape == valid.shape == (5, k) and rows.dtype == torch.int64 and valid.dtype == torch.bool
            assert int(ctr) == ctr0 + step + 1
            er, ev = S.select(cs, cap, num, 9, ctr0 + step)
            assert np.array_equal(valid.cpu().numpy(), ev), (cs, step)
            assert np.array_equal(rows.cpu().numpy(), er), (cs, step)
            # what the loss relies on, stated on the device's own output
            r, v = rows.cpu().numpy(), valid.cpu().numpy()
            assert (r[~v] == 0).all()
            for b, c in enumerate(cs):
                m = min(c, cap)
                n = min(k, m)
                assert v[b, :n].all() and not v[b, n:].any()
                assert len(set(r[b, :n].tolist())) == n and (n == 0 or (0 <= r[b, :n].min() and r[b, :n].max() < m))


def test_empty_calls_leave_ctr(device):
    from dpfm_amd import ops
    ctr = torch.full((1,), 17, dtype=torch.int64, device=device)
    counts = torch.tensor([5, 600], dtype=torch.int64, device=device)
    rows, valid = ops.nce_select(counts, 64, 0, 9, ctr)  # num = 0
    assert rows.shape == valid.shape == (2, 0)
    rows, valid = ops.nce_select(counts, 0, 8, 9, ctr)   # cap = 0: k = 0
    assert rows.shape == valid.shape == (2, 0)
    rows, valid = ops.nce_select(counts[:0], 64, 8, 9, ctr)  # B = 0
    assert rows.shape == valid.shape == (0, 8)
    assert int(ctr) == 17
