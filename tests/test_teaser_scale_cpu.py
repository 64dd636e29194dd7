"""(f2) TEASER++ with scale estimation, host stages (pk_teaser_solve_scaled) against the numpy
restatement in _teaser_scale_ref.py, on host inputs — no GPU needed: the scale and the scaled graph
come from the reference (their device twins are tested in test_teaser_scale_gpu.py).

  * scale = NULL and scale = all ones equal pk_teaser_solve bit for bit;
  * planted scaled crops: the clique is the reference's max k-core / a clique of the maximum size;
    T within 1e-9 (the project's f2 tolerance) of the reference's scaled GNC-TLS + voting on that
    clique, the same inlier counts; the planted scale, rotation and translation are recovered;
  * degenerate crops (0, 1 correspondences, two coincident source points): invalid, identity,
    scale 1;
  * the ctypes table holds the four new entry points.
"""
import functools

import numpy as np
import pytest

from oracle import dpfm_oracle as O
from test_teaser_cpu import pack_bits, planted

import _teaser_scale_ref as R

BETA = 0.1  # 2 noise_bound sqrt(cbar2), noise_bound = 0.05
CASES = [(64, 0.5, 1.7), (130, 0.3, 0.6), (200, 0.15, 2.5), (150, 0.8, 1.3)]


def params():
    from dpfm_amd import _lib
    return _lib.TeaserParams(0.05, 1.0, 1.4, 1e-12, 0.5, 100, 0, 2_000_000)


def host_inputs(crops, nmax, graphs):
    a = np.concatenate([c[0] for c in crops] + [np.zeros((1, 3))])
    b = np.concatenate([c[1] for c in crops] + [np.zeros((1, 3))])
    off = np.concatenate([[0], np.cumsum([c[0].shape[0] for c in crops])]).astype(np.int64)
    adj = np.stack([pack_bits(g, nmax) for g in graphs])
    deg = np.stack([np.pad(g.sum(1).astype(np.int64), (0, nmax - g.shape[0])) for g in graphs]).astype(np.int32)
    return a, b, off, adj, deg


@functools.lru_cache(maxsize=None)
def scaled_case(n, frac, s):
    """One planted crop with the reference's vote and scaled graph (computed once, shared)."""
    rng = np.random.default_rng(1000 + n)
    a, b, Tt, _ = R.planted_scaled(rng, n, frac, s)
    v = R.scale_vote(a, b, BETA)
    g = R.scaled_graph(a, b, BETA, v["scale"])
    for x in (a, b, g):
        x.setflags(write=False)
    return a, b, Tt, v, g


@pytest.mark.parametrize("frac,n,mode", [(0.8, 150, 2), (0.3, 70, 1), (0.15, 90, 1)])
def test_unit_scale_equals_unscaled_solve(frac, n, mode):
    from dpfm_amd import ops
    rng = np.random.default_rng(int(frac * 100) + n)
    crops = [planted(rng, n - 7 * k, frac) for k in range(3)]
    graphs = [O.teaser_graph(c[0], c[1], BETA) for c in crops]
    a, b, off, adj, deg = host_inputs(crops, n, graphs)
    base = ops.teaser_solve_host(a, b, off, n, adj, deg, params(), threads=4)
    assert (base[3][:, 0] == 1).all() and (base[3][:, 1] == mode).all()
    import ctypes
    c = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    from dpfm_amd import _lib
    for scale in (None, np.ones(3)):
        T, clique, size, info = np.zeros((3, 4, 4)), np.zeros((3, n), np.int32), np.zeros(3, np.int32), np.zeros(
            (3, 4), np.int32)
        st = _lib.lib().pk_teaser_solve_scaled(c(a), c(b), c(off), 3, n, c(adj), c(deg), ctypes.byref(params()), 4,
                                               None if scale is None else c(scale), c(T), c(clique), c(size), c(info))
        assert st == 0
        for got, ref in zip((T, clique, size, info), base):
            np.testing.assert_array_equal(got, ref)
    ones = ops.teaser_solve_host(a, b, off, n, adj, deg, params(), threads=4, scale=np.ones(3))
    for got, ref in zip(ones, base):
        np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("n,frac,s", CASES)
def test_scaled_host_matches_reference(n, frac, s):
    from dpfm_amd import ops
    a, b, Tt, v, g = scaled_case(n, frac, s)
    sh = v["scale"]
    assert v["status"] == 1
    ha, hb, off, adj, deg = host_inputs([(a, b)], n, [g])
    T, clique, size, info = ops.teaser_solve_host(ha, hb, off, n, adj, deg, params(), threads=1, scale=np.array([sh]))
    core = O.core_numbers(g)
    mode = 2 if core.max() > int(0.5 * n) else 1
    C = clique[0, :size[0]]
    assert info[0, 0] == 1 and info[0, 1] == mode, info[0]
    if mode == 2:
        np.testing.assert_array_equal(C, np.flatnonzero(core >= core.max()))
    else:
        assert size[0] == O.max_clique_size(g)
        assert (g[np.ix_(C, C)] | np.eye(len(C), dtype=bool)).all()
    To, rin, tin = R.from_clique_scaled(a, b, C, sh)
    print(f"n={n} s={s}: scale err {abs(sh - s) / s:.3g}, |T - ref| {np.abs(T[0] - To).max():.3g}, "
          f"|dR| {np.abs(T[0][:3, :3] - Tt[:3, :3]).max():.3g}, |dt| {np.abs(T[0][:3, 3] - Tt[:3, 3]).max():.3g}")
    np.testing.assert_allclose(T[0], To, atol=1e-9)
    assert info[0, 2] == rin and info[0, 3] == tin
    assert abs(sh - s) / s < 1e-3
    assert np.abs(T[0][:3, :3] - Tt[:3, :3]).max() < 5e-3 and np.abs(T[0][:3, 3] - Tt[:3, 3]).max() < 0.05


def test_scaled_host_degenerate():
    from dpfm_amd import ops
    twin = (np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))
    crops = [(np.zeros((0, 3)), np.zeros((0, 3))), (np.ones((1, 3)), np.ones((1, 3))), twin]
    votes = [R.scale_vote(a, b, BETA) for a, b in crops]
    scale = np.array([v["scale"] for v in votes])
    assert (scale == 1.0).all() and all(v["status"] == 0 for v in votes)
    graphs = [R.scaled_graph(a, b, BETA, 1.0) for a, b in crops]
    assert not graphs[2].any()
    ha, hb, off, adj, deg = host_inputs(crops, 8, graphs)
    T, clique, size, info = ops.teaser_solve_host(ha, hb, off, 8, adj, deg, params(), threads=2, scale=scale)
    for k in range(3):
        assert info[k, 0] == 0 and np.array_equal(T[k], np.eye(4)), (k, info[k])


def test_signatures_hold_the_scale_entry_points():
    from dpfm_amd import _lib
    for name in ("pk_teaser_scale_work_size", "pk_teaser_scale", "pk_teaser_graph_scaled", "pk_teaser_solve_scaled"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.RESTYPES["pk_teaser_scale_work_size"] is _lib._I64
