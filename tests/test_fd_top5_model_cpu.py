"""CPU checks of the top-5 feature-distance tests' own tools: the exact fp32 fma of
tests/_util.fd_emulate against libm's fmaf, the host model of fd_top5_kernel's selection
(tests/_fd_top5_model.py) against the plain stable top-5 of the same distances, and the path
conditions that each clustered input must meet before it means anything on the device."""
import ctypes

import numpy as np
import pytest
import torch

import _fd_top5_model as M
from _util import fd_emulate, fd_expected_topk, fma_f32


def _libm_fmaf():
    try:
        f = ctypes.CDLL("libm.so.6").fmaf
    except (OSError, AttributeError):
        return None
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return f


def test_fma_f32_equals_libm_fmaf():
    """200k random triples over a wide exponent range, and 50k triples whose product sits exactly
    on an f32 rounding midpoint with a tiny c on either side (the double rounding of
    f32(f64(a b + c)) goes wrong on thousands of these): fma_f32 is bit-equal to fmaf on all."""
    fmaf = _libm_fmaf()
    if fmaf is None:
        pytest.skip("libm.so.6 cannot be loaded")
    rng = np.random.default_rng(7)
    n = 200_000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c[: n // 2] = (-(a[: n // 2].astype(np.float64) * b[: n // 2]) * (1 + rng.standard_normal(n // 2) * 1e-6)).astype(
        np.float32)  # cancellation
    m = 50_000
    k, mm = rng.integers(1, 1 << 12, m), rng.integers(1, 1 << 13, m)
    am = (1 + k * 2.0 ** -12).astype(np.float32)
    bm = (1 + mm * 2.0 ** -13).astype(np.float32)
    cm = (rng.choice([-1.0, 1.0], m) * 2.0 ** -rng.integers(60, 101, m).astype(np.float64)).astype(np.float32)
    for aa, bb, cc, what in [(a, b, c, "random"), (am, bm, cm, "midpoint")]:
        got = fma_f32(aa, bb, cc)
        ref = np.array([fmaf(x, y, z) for x, y, z in zip(aa.tolist(), bb.tolist(), cc.tolist())], np.float32)
        bad = np.nonzero(got.view(np.int32) != ref.view(np.int32))[0]
        assert bad.size == 0, (what, bad.size, aa[bad[:3]], bb[bad[:3]], cc[bad[:3]])
    naive = (am.astype(np.float64) * bm + cm).astype(np.float32)
    assert (naive != fma_f32(am, bm, cm)).sum() > 1000  # the crafted set does hit the double rounding


def test_top1_plan_and_wave_tiles():
    assert M.top1_plan(192, 1024, 128) == (1, 1) and M.top1_plan(191, 1024, 128) == (1, 2)
    assert M.top1_plan(25, 1024, 1000) == (8, 1)
    assert M.top1_plan(2, 1024, 128) == (1, 4) and M.top1_plan(3, 1024, 128) == (1, 4)
    assert M.top1_plan(32, 1024, 1024) == (8, 1)  # configs[1] infer
    assert M.wave_tiles(1024, 1) == [(8 * w, 8 * w + 8) for w in range(8)]
    assert M.wave_tiles(1019, 1) == M.wave_tiles(1024, 1)
    assert M.wave_tiles(1024, 4) == [(2 * q, 2 * q + 2) for q in range(32)]
    assert M.wave_tiles(40, 1) == [(0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 3)]


@pytest.mark.parametrize("name", sorted(M.INPUTS))
def test_model_equals_reference_and_reaches_its_path(name):
    """The model's five (the kernel's algorithm) equal the stable top-5 of the same emulated
    distances at RS = 1 and RS = 4, and at RS = 1 the input's path facts meet its conditions."""
    ex, ey, n1, n2, d, ei, ev = M.case(name)
    for RS in (1, 4):
        gi, gv, facts = M.crop_result(name, RS)
        np.testing.assert_array_equal(gi, ei)
        np.testing.assert_array_equal(gv.view(np.int32), ev.view(np.int32))
        if RS == 1 and name not in M.NO_CONDITIONS:
            M.check_conditions(name, facts[0][0])
    if name == "random":  # what the suite had before: next to nothing on E3b / E3c
        f = M.crop_result(name, 1)[2][0][0]
        assert f["task_total"] < 64 and all(r is None for r in f["reason"])


def test_conditions_see_a_clamped_candidate():
    """check_conditions fails where an over-full or overflowing column holds a clamped candidate:
    list16 and an overflow input with 16 crop columns replaced by CAD rows (the rounded distance
    of a copy is about 0: at or below the clamp in some of them, a few 1e-6 in the others)."""
    for name in ("list16", "overflow_eps"):
        ex, ey, n1, n2 = M.case(name)[:4]
        M.check_conditions(name, M.crop_result(name, 1)[2][0][0])
        ey = ey.copy()
        ey[:16] = ex[40:56]
        d = fd_emulate(ex, M.EYE, ey, n1, n2)
        hit = d.min(0) <= np.float32(1e-30)
        assert 1 <= hit.sum() <= 16 and not hit[16:].any()
        f = M.top5_block(d, 1, 0, 0, n2)[1]
        np.testing.assert_array_equal(f["cand_clamped"], hit)
        with pytest.raises(AssertionError):
            M.check_conditions(name, f)


def test_top5_rejects_more_rows_than_a_task_entry_holds():
    """The mode-0 top-5 takes V1max <= 2^24 (posekern.h): one more row is refused by the size query
    and by the entry point, before any pointer is read; top-1 and the bf16 modes are not bound."""
    from dpfm_amd import _lib
    lib = _lib.lib()
    big = (1 << 24) + 1
    assert lib.pk_feat_dist_work_size(1, big, 16, 5, 0) == -1
    assert lib.pk_feat_dist_work_size(1, big - 1, 16, 5, 0) > 0
    assert lib.pk_feat_dist_work_size(1, big, 16, 1, 0) > 0 and lib.pk_feat_dist_work_size(1, big, 16, 5, 1) > 0
    st = lib.pk_feat_dist_topk(None, 32, None, None, 32, None, None, 1, big, 16, 5, 0, None, 0, None, None, None)
    assert st == 1000  # PK_ERR_ARG


def test_builder_figures():
    """The figures the inputs were built for, beyond their conditions: an overflowing block's task
    total is twice the list and more, with at most 14 candidates in a column; the merge inputs
    reach an exactly full short list; the eps = 0 inputs at RS = 4 still list streams (exact ties
    inside a wave's two tiles). (The model's results are shared with the test above.)"""
    for name in M.INPUTS:
        if name.startswith("overflow"):
            f = M.crop_result(name, 1)[2][0][0]
            assert 3500 <= f["task_total"] <= 3584 and f["ncand"].max() <= 14, (name, f["task_total"], f["ncand"].max())
    assert any((M.crop_result(n, 1)[2][0][0]["nbelow"] == M.K_X).any() for n in M.INPUTS if n.startswith("merge"))
    for name in ("overflow_tie", "overflow_pair_tie_1019", "merge_tie", "short8_tie_1019", "ties_wide", "ties_wide_1019"):
        parts = M.crop_result(name, 4)[2][0]
        assert min(int(f["nlisted"].sum()) for f in parts) > 0, name
    for name in ("ties_wide", "ties_wide_1019"):  # fives that hold equal values from different row parts
        ei, ev = M.case(name)[5:]
        assert ((ev[:, 1:] == ev[:, :-1]) & (ei[:, 1:] // 256 != ei[:, :-1] // 256)).sum() >= 10, name


def _spectral(V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(V, 32, generator=g) * torch.linspace(1.5, 0.3, 32)[None, :]


@pytest.mark.parametrize("n1,n2,RS", [(1024, 200, 1), (1024, 128, 4), (300, 130, 1), (3, 40, 1), (17, 9, 1), (5, 7, 2)])
def test_model_on_spectral_and_ragged(n1, n2, RS):
    """Spectral-decay features under a dense C, ragged sizes (fewer than five rows, waves without a
    tile), and copies of crop columns among the CAD rows (distances at or below the clamp)."""
    g = torch.Generator().manual_seed(n1 + n2)
    ex, ey = _spectral(1024, 300 + n1).numpy().copy(), _spectral(max(n2, 1), 400 + n2).numpy()
    C = (torch.eye(30) + 0.3 * torch.randn(30, 30, generator=g)).numpy()
    d = fd_emulate(ex, C, ey, n1, n2)
    ei, ev = fd_expected_topk(d, 5)
    gi, gv, _ = M.top5_crop(d, RS)
    np.testing.assert_array_equal(gi, ei)
    np.testing.assert_array_equal(gv, ev)
    if n1 >= 300:  # exact copies, each duplicated at a later row: clamped and tied
        ex[n1 // 2: n1 // 2 + 10] = ey[:10]
        ex[n1 - 10: n1] = ey[:10]
        d = fd_emulate(ex, np.eye(30, dtype=np.float32), ey, n1, n2)
        ei, ev = fd_expected_topk(d, 5)
        gi, gv, facts = M.top5_crop(d, RS)
        np.testing.assert_array_equal(gi, ei)
        np.testing.assert_array_equal(gv, ev)
        assert any(r == "clamp" for cg in facts for f in cg for r in f["reason"])
