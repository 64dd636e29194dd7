"""CPU: pins the fp64 ZoomOut reference (tests/_zoomout_ref.py) that the device kernels are held to
(tests/test_zoomout_gpu.py), on analytic Neumann eigenfunctions of a rectangle."""
import numpy as np
import pytest

import _zoomout_ref as R

N1, N2, STEP = 601, 333, 5
SEEDS = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def cases():
    return {s: R.rect_case(s, N1, N2) for s in SEEDS}


def test_generator_bases_are_orthonormal_and_ordered():
    ab = R.rect_modes()
    lam = ab[:, 0] ** 2 + (ab[:, 1] / R.H) ** 2
    assert len(ab) == 64 and tuple(ab[0]) == (0, 0) and np.all(np.diff(lam) >= 0)
    # a midpoint-rule Gram matrix of the 64 modes under the area measure is the identity (the rule is
    # exact for these cosines up to aliasing at multiples of 2 * 64)
    g = (np.arange(64) + 0.5) / 64
    P = np.stack(np.meshgrid(g, g * R.H, indexing="ij"), -1).reshape(-1, 2)
    Phi = R.rect_eigenfunctions(P)
    assert np.abs(Phi.T @ Phi * (R.H / len(P)) - np.eye(64)).max() < 1e-12


def test_k_final_30_is_the_plain_argmin(cases):
    c = cases[1]
    C, p = R.zoomout(c["ex"], c["ey"], c["mass"], c["C0"], N1, N2, k_final=30, step=3)
    E = c["ex"].astype(np.float64)[:, :30] @ c["C0"].astype(np.float64).T
    d = ((E[:, None, :] - c["ey"].astype(np.float64)[None, :, :30]) ** 2).sum(-1)
    assert np.array_equal(p, d.argmin(0))
    assert np.array_equal(C, c["C0"].astype(np.float64))


def grid_basis(n=16):
    """f32 modes on the n x n midpoint grid with mass H / n^2: exactly mass-orthonormal in exact
    arithmetic (the midpoint rule integrates products of these cosines exactly below order 2 n)."""
    g = (np.arange(n) + 0.5) / n
    P = np.stack(np.meshgrid(g, g * R.H, indexing="ij"), -1).reshape(-1, 2)
    return R.rect_eigenfunctions(P).astype(np.float32), np.full(n * n, R.H / (n * n), np.float32)


@pytest.mark.parametrize("step", [1, 5, 34])
def test_identity_is_a_fixed_point(step):
    """Y = X with C0 = I: every size's point map is the identity and every size's C is I."""
    ex, mass = grid_basis()
    n = len(ex)
    C = np.eye(30)
    ks = R.schedule(64, step)
    for it, k in enumerate(ks):
        p = R.point_map(ex, ex, C, n, n, k)
        assert np.array_equal(p, np.arange(n)), k
        if it + 1 < len(ks):
            C = R.project(ex, ex, mass, p, n, ks[it + 1])
            assert np.abs(C - np.eye(ks[it + 1])).max() < 1e-5
    Cf, pf = R.zoomout(ex, ex, mass, np.eye(30), n, n, 64, step)
    assert np.array_equal(pf, np.arange(n)) and Cf.shape == (64, 64)


def test_schedule():
    assert R.schedule(30, 4) == [30]
    assert R.schedule(64, 34) == [30, 64]
    assert R.schedule(47, 5) == [30, 35, 40, 45, 47]
    assert R.schedule(64, 1) == list(range(30, 65))


@pytest.mark.parametrize("seed", SEEDS)
def test_refinement_lowers_the_map_error(cases, seed):
    c = cases[seed]
    naive = R.map_error(c, R.point_map(c["ex"], c["ey"], c["C0"], N1, N2, 30))
    C, p = R.zoomout(c["ex"], c["ey"], c["mass"], c["C0"], N1, N2, 64, STEP)
    refined = R.map_error(c, p)
    print(f"seed {seed}: naive {naive:.4f} refined {refined:.4f} ratio {refined / naive:.3f}")
    assert C.shape == (64, 64) and p.shape == (N2,) and p.max() < N1
    assert refined <= 0.85 * naive


@pytest.mark.parametrize("seed", SEEDS)
def test_near_ties_are_rare(cases, seed):
    """At every size of the schedule, the columns whose fp64 best / second-best gap is under the
    f32 acceptance bound tau (the only columns where the device may pick another row) are <= 2 %."""
    c = cases[seed]
    C = c["C0"].astype(np.float64)
    ks = R.schedule(64, STEP)
    for it, k in enumerate(ks):
        s = R.scores(c["ex"], c["ey"], C, N1, N2, k)
        two = np.partition(s, 1, axis=0)[:2]
        share = float((two[1] - two[0] < R.tau(c["ex"], c["ey"], C, N1, N2, k)).mean())
        print(f"seed {seed} k {k}: near-tie share {share:.4f}")
        assert share <= 0.02, (k, share)
        if it + 1 < len(ks):
            C = R.project(c["ex"], c["ey"], c["mass"], s.argmin(0), N2, ks[it + 1])
