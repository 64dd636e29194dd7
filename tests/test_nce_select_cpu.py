"""Pins tests/_nce_select_model.py (the host model test_nce_select_gpu.py holds pk_nce_select to,
bit for bit) on the properties the draw is used for: a valid prefix of distinct in-range rows, a
function of (seed, ctr, crop), and uniform inclusion. The model is deterministic: a failure here
is a wrong model or a biased draw, never chance."""
import numpy as np
import pytest

import _nce_select_model as S

CASES = [(0, 64, 8), (1, 64, 8), (2, 64, 8), (5, 64, 8), (8, 64, 8), (9, 64, 8), (64, 64, 8), (71, 64, 8),
         (0, 64, 512), (1, 64, 512), (63, 64, 512), (64, 64, 512), (71, 64, 512),
         (511, 2000, 512), (512, 2000, 512), (513, 2000, 512), (1500, 2000, 512), (2000, 2000, 512),
         (2007, 2000, 512), (1500, 2000, 8), (2007, 2000, 8), (3, 2000, 0), (-4, 64, 8)]


def test_splitmix64_known_values():
    """The published splitmix64 stream from state 0: the first outputs of the reference generator."""
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF
    assert S.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("count,cap,num", CASES)
def test_valid_prefix_of_distinct_rows_in_range(count, cap, num):
    m = max(min(count, cap), 0)
    for crop, ctr in ((0, 0), (3, 41)):
        rows, valid = S.select_crop(count, cap, num, 9, ctr, crop)
        n = min(num, m)
        assert rows.shape == valid.shape == (min(num, cap),)
        assert valid[:n].all() and not valid[n:].any()
        assert (rows[n:] == 0).all()
        assert len(set(rows[:n].tolist())) == n
        assert n == 0 or (rows[:n].min() >= 0 and rows[:n].max() < m)


def test_full_draw_is_a_permutation():
    for m in (1, 2, 3, 64, 65, 511, 512, 513):
        rows, valid = S.select_crop(m, 2000, 2000, 7, 5, 1)
        assert valid[:m].all() and sorted(rows[:m].tolist()) == list(range(m))


def test_draw_depends_on_seed_ctr_and_crop_only():
    base = S.select([1500] * 3, 2000, 512, 9, 0)
    again = S.select([1500] * 3, 2000, 512, 9, 0)
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1])
    assert not np.array_equal(base[0][0], base[0][1]) and not np.array_equal(base[0][1], base[0][2])  # crops
    assert not np.array_equal(base[0], S.select([1500] * 3, 2000, 512, 9, 1)[0])   # ctr
    assert not np.array_equal(base[0], S.select([1500] * 3, 2000, 512, 10, 0)[0])  # seed
    # a crop's draw does not depend on its neighbours' counts
    assert np.array_equal(base[0][1], S.select([3, 1500, 0], 2000, 512, 9, 0)[0][1])


@pytest.mark.parametrize("count,num", [(1500, 512), (2000, 512), (513, 512), (700, 8)])
def test_inclusion_is_uniform(count, num):
    """Over ctr = 0..1999 (seed 9, crop 0) every row's inclusion count is Binomial(2000, num / count)
    under a uniform draw: |z| <= 6 for every row and chi^2 / dof <= 1 + 5 sqrt(2 / dof), dof = count - 1
    (the counts sum to 2000 num)."""
    T = 2000
    hits = np.zeros(count, dtype=np.int64)
    for ctr in range(T):
        rows, valid = S.select_crop(count, 2000, num, 9, ctr, 0)
        hits[rows[valid]] += 1
    assert hits.sum() == T * num
    p = num / count
    z = (hits - T * p) / np.sqrt(T * p * (1 - p))
    dof = count - 1
    chi = float((z ** 2).sum()) / dof
    print(f"nce_select uniformity count={count} num={num}: max|z|={np.abs(z).max():.2f} (limit 6) "
          f"chi2/dof={chi:.3f} (limit {1 + 5 * np.sqrt(2 / dof):.3f})")
    assert np.abs(z).max() <= 6
    assert chi <= 1 + 5 * np.sqrt(2 / dof)
