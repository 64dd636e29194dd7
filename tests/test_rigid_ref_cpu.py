"""Pins tests/_rigid_ref.py, the fp64 reference test_rigid_fit_gpu.py holds the device's 4-point
rigid fit (csrc/rigid.hpp) to, without a GPU:

  * umeyama_ref against the C oracle's oc_umeyama (one-sided Jacobi SVD), 256 draws of every
    family that determines the rotation: |R - R_c| <= 64 x the reference's own sensitivity to a
    one-ulp change of its inputs, + 1e-14;
  * the reference meets the structural, optimality and residual bars it sets, on every family;
  * every `unique` family keeps mu >= 1e-6 on all of its draws with the seed the tests share
    (a seed that breaks this is changed, not the cap), and there 1024 eps / mu, the rotation bar,
    is never below 4 x the sensitivity: the bar cannot be tighter than the problem;
  * the planar RANSAC cases of test_corr_pose_gpu.py have one winner: the oracle's best two
    hypotheses differ in fitness, or in rmse by more than 1e-6.
"""
import numpy as np
import pytest

import _rigid_ref as RR
from _util import cp


@pytest.fixture(scope="module")
def ref_fits():
    return {name: RR.umeyama_ref(s, d) for name, (s, d, _) in RR.all_draws().items()}


def test_families_are_the_ones_the_gpu_test_expects():
    fam = RR.draws()
    assert len(fam) == 23 and sum(u for _, _, u in fam.values()) == 17
    for name, (s, d, _) in fam.items():
        assert s.shape == d.shape == (RR.PER_FAMILY, 4, 3), name
    s = fam["one_repeat"][0]
    assert (s[:, 0] == s[:, 1]).all() and (fam["integer_plane"][0][..., 2] == 900.0).all()
    assert (np.linalg.det(ref_S(fam["mirrored"])) < 0).mean() > 0.9   # det S < 0: the sign fix is taken


def ref_S(family):
    return RR.umeyama_ref(family[0], family[1])[2]


def test_unique_families_determine_the_rotation(ref_fits):
    for name, (s, d, unique) in RR.all_draws().items():
        mu = ref_fits[name][5]
        if not unique:
            continue
        assert mu.min() >= RR.MU_MIN, (name, int(np.argmin(mu)), float(mu.min()))
        sens = RR.family_sensitivity(name, s, d)
        ratio = sens * mu / RR.EPS
        print(f"{name:22s} mu min {mu.min():.2e}  sensitivity mu / eps max {ratio.max():.1f}")
        assert (1024 * RR.EPS / mu >= 4 * sens).all(), (name, int(np.argmax(ratio)), float(ratio.max()))


def test_reference_matches_c_oracle(coracle, ref_fits):
    for name, (s, d, unique) in RR.all_draws().items():
        if not unique:
            continue
        R = ref_fits[name][0]
        Rc = np.zeros((s.shape[0], 9))
        tc = np.zeros((s.shape[0], 3))
        for i in range(s.shape[0]):
            coracle.oc_umeyama(cp(s[i]), cp(d[i]), 4, cp(Rc[i]), cp(tc[i]))
        err = np.abs(R.reshape(-1, 9) - Rc).max(1)
        bar = 64 * RR.family_sensitivity(name, s, d) + 1e-14
        i = int(np.argmax(err / bar))
        print(f"{name:22s} |R - R_c| {err[i]:.2e} / {bar[i]:.2e} at draw {i} (mu {ref_fits[name][5][i]:.2e})")
        assert (err <= bar).all(), (name, i, float(err[i]), float(bar[i]))


def test_reference_meets_its_own_bars(ref_fits):
    fails = []
    for name, (s, d, unique) in RR.all_draws().items():
        R, t = ref_fits[name][:2]
        fails += RR.check_fits(name, s, d, R, t, unique)
    assert not fails, "\n".join(fails)


def planar_scores(coracle, trial):
    """(fitness, rmse) of every hypothesis of a planar trial: one oc_ransac call per explicit
    hypothesis row."""
    data_seed, seed = RR.PLANAR_TRIALS[trial]
    cad, pc, corres, _, _ = RR.planar_ransac_case(data_seed)
    n = corres.shape[0]
    out = np.zeros((RR.PLANAR_H, 2))
    T, st = np.zeros(16), np.zeros(3)
    for h in range(RR.PLANAR_H):
        row = np.array([coracle.oc_hyp_index(seed, h, j, n) for j in range(4)], dtype=np.int32)
        coracle.oc_ransac(cp(cad), cp(pc), cp(corres), n, cp(row), 0, 1, RR.PLANAR_MAX_DIST, cp(T), cp(st))
        out[h] = st[:2]
    return out


@pytest.mark.parametrize("trial", range(len(RR.PLANAR_TRIALS)))
def test_planar_ransac_cases_have_one_winner(coracle, trial):
    sc = planar_scores(coracle, trial)
    order = sorted(range(len(sc)), key=lambda h: (-sc[h, 0], sc[h, 1], h))
    a, b = sc[order[0]], sc[order[1]]
    print(f"trial {trial}: best {order[0]} {a.tolist()}, second {order[1]} {b.tolist()}")
    assert a[0] >= 0.2                      # an all-inlier draw exists: the pose is found
    assert a[0] != b[0] or b[1] - a[1] > 1e-6
