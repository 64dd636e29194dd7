"""(f2) TEASER++ scale estimation on the device (csrc/teaser_scale.hip) against the numpy
restatement in _teaser_scale_ref.py:

  * the vote (emit -> stable radix sort -> segmented fp64 scans -> argmin) on a ragged batch and on
    one crop of 600 pairs (3.6e5 endpoints: many tiles, every radix digit): the reference's
    minimum is first shown to be separated (>= 1e-7 relative from every candidate whose estimate
    differs by more than 1e-9 relative; the fp64 reordering error of the cost is ~1e-11), then the
    device scale is within 1e-9 relative (same winner, another summation order: ~4 K 2^-53) and
    the consensus sizes are equal;
  * equal keys and the va == 0 rule: an integer lattice with a duplicated point, b = 2 a exactly;
  * a crop whose keys share their six low bytes (those radix passes are skipped for it);
  * reproducibility: bitwise equal results whatever the workspace held, and whatever the chunking;
  * the scaled graph bit-exact given the device's own scale, padding rows included;
  * end to end: ops.teaser(estimate_scaling=True) = the host solve fed the downloaded device graph
    and scale; the upstream-default RobustRegistrationSolver recovers a planted scaled pose;
  * the default path (no scale estimation) is unchanged.
"""
import functools

import numpy as np
import pytest
import torch

from test_teaser_cpu import planted, run_host
from test_teaser_scale_cpu import BETA, params

import _teaser_scale_ref as R

pytestmark = pytest.mark.gpu

RAGGED = [(64, 0.5, 1.7), (130, 0.3, 0.6), (0, 1.0, 1.0), (1, 1.0, 1.0), (2, 1.0, 1.3), (200, 0.15, 2.5),
          (257, 0.4, 1.3)]


@functools.lru_cache(maxsize=None)
def batch(which):
    """(crops, reference votes) of the ragged batch / the single 600-pair crop; computed once."""
    rng = np.random.default_rng(7)
    spec = RAGGED if which == "ragged" else [(600, 0.4, 1.7)]
    crops = [R.planted_scaled(rng, n, f, s)[:2] for n, f, s in spec]
    for a, b in crops:
        a.setflags(write=False)
        b.setflags(write=False)
    return crops, [R.scale_vote(a, b, BETA) for a, b in crops]


@functools.lru_cache(maxsize=None)
def lattice():
    """120 integer lattice points of [0, 6]^3 (many equal distances), one of them twice; b = 2 a."""
    rng = np.random.default_rng(11)
    grid = np.stack(np.meshgrid(*[np.arange(7.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    a = grid[rng.permutation(grid.shape[0])[:119]]
    a = np.concatenate([a, a[17:18]])
    return a, 2.0 * a


def pack(crops, device):
    a = np.concatenate([c[0] for c in crops] + [np.zeros((1, 3))])
    b = np.concatenate([c[1] for c in crops] + [np.zeros((1, 3))])
    off = np.concatenate([[0], np.cumsum([c[0].shape[0] for c in crops])]).astype(np.int64)
    return torch.from_numpy(a).to(device), torch.from_numpy(b).to(device), torch.from_numpy(off).to(device)


@pytest.mark.parametrize("which", ["ragged", "single600"])
def test_scale_vote_matches_reference(device, which):
    from dpfm_amd import ops
    crops, votes = batch(which)
    nmax = max(c[0].shape[0] for c in crops)
    a, b, off = pack(crops, device)
    scale, info = ops.teaser_scale(a, b, off, nmax, BETA)
    scale, info = scale.cpu().numpy(), info.cpu().numpy()
    for k, ((ca, _), v) in enumerate(zip(crops, votes)):
        if ca.shape[0] < 2:
            assert scale[k] == 1.0 and info[k, 0] == 0, (k, scale[k], info[k])
            continue
        margin = R.vote_margin(v)
        print(f"crop {k} n={ca.shape[0]}: margin {margin:.3g}, ref {v['scale']!r}, dev {scale[k]!r}, "
              f"rel {abs(scale[k] - v['scale']) / v['scale']:.3g}, card {v['card']} / {info[k, 1]}")
        assert margin >= 1e-7, (k, margin)  # precondition on the reference alone
        assert abs(scale[k] - v["scale"]) <= 1e-9 * v["scale"], (k, scale[k], v["scale"])
        assert info[k, 0] == 1 and info[k, 1] == v["card"], (k, info[k], v["card"])


def test_scale_vote_equal_keys_and_duplicate_point(device):
    from dpfm_amd import ops
    la, lb = lattice()
    v = R.scale_vote(la, lb, 0.5)  # noise_bound 0.25
    a, b, off = pack([(la, lb)], device)
    scale, info = ops.teaser_scale(a, b, off, la.shape[0], 0.5)
    assert float(scale[0]) == 2.0
    assert v["scale"] == 2.0 and int(info[0, 0]) == 1 and int(info[0, 1]) == v["card"]
    assert v["card"] == la.shape[0] * (la.shape[0] - 1) // 2 - 1  # every pair but the duplicate's


def test_scale_vote_with_skipped_radix_passes(device):
    """Three collinear points at 0, 1, 2 and b = 2 a, beta = 0.5: the endpoints 2 -+ 0.5 / va are
    short binary fractions, so the six low bytes of every key are zero and those radix passes are
    skipped (the records stay in the first buffer until a live pass moves them), next to a crop
    whose passes are all live."""
    from dpfm_amd import ops
    la = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    ends = np.array([2 - 0.5, 2 + 0.5, 2 - 0.25, 2 + 0.25])
    assert (ends.view(np.uint64) & np.uint64(0xFFFFFFFFFFFF) == 0).all()  # constant low digits
    other = batch("ragged")[0][0]
    a, b, off = pack([(la, 2.0 * la), other], device)
    scale, info = ops.teaser_scale(a, b, off, other[0].shape[0], 0.5)
    v = R.scale_vote(la, 2.0 * la, 0.5)
    assert v["scale"] == 2.0 and v["card"] == 3
    assert float(scale[0]) == 2.0 and info[0].tolist() == [1, 3]
    vo = R.scale_vote(other[0], other[1], 0.5)
    assert R.vote_margin(vo) >= 1e-7  # 1.4e-4: the precondition of the 1e-9 bound, as above
    assert abs(float(scale[1]) - vo["scale"]) <= 1e-9 * vo["scale"] and info[1].tolist() == [1, vo["card"]]


def test_scale_vote_reproducible_for_any_workspace(device):
    from dpfm_amd import _lib, ops
    crops, _ = batch("ragged")
    nmax = max(c[0].shape[0] for c in crops)
    a, b, off = pack(crops, device)
    nbytes = int(_lib.lib().pk_teaser_scale_work_size(len(crops), nmax))
    outs = []
    for fill in (0xFF, 0x00):
        work = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
        scale, info = ops.teaser_scale(a, b, off, nmax, BETA, work=work)
        adj, deg = ops.teaser_graph(a, b, off, nmax, BETA, scale=scale)
        outs.append((scale, info, adj, deg))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_teaser_scaled_independent_of_chunking(device, monkeypatch):
    from dpfm_amd import ops
    crops, _ = batch("ragged")
    a, b, off = pack(crops, device)
    whole = ops.teaser(a, b, off, threads=4, estimate_scaling=True)
    monkeypatch.setattr(ops, "TEASER_SCALE_WORK_CAP", 1)  # one crop per chunk
    chunked = ops.teaser(a, b, off, threads=4, estimate_scaling=True)
    assert len(whole) == 5
    for x, y in zip(whole, chunked):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("which", ["ragged", "lattice"])
def test_scaled_graph_bitexact(device, which):
    from dpfm_amd import ops
    from test_teaser_cpu import pack_bits
    crops, beta = (batch("ragged")[0], BETA) if which == "ragged" else ([lattice()], 0.5)
    nmax = max(c[0].shape[0] for c in crops) + 9  # padding rows in every crop
    a, b, off = pack(crops, device)
    scale, _ = ops.teaser_scale(a, b, off, nmax, beta)
    adj, deg = ops.teaser_graph(a, b, off, nmax, beta, scale=scale)
    adj, deg, scale = adj.cpu().numpy().view(np.uint64), deg.cpu().numpy(), scale.cpu().numpy()
    for k, (ca, cb) in enumerate(crops):
        ref = R.scaled_graph(ca, cb, beta, scale[k])
        np.testing.assert_array_equal(adj[k], pack_bits(ref, nmax), err_msg=f"crop {k}")
        np.testing.assert_array_equal(deg[k, :ca.shape[0]], ref.sum(1))
        assert (deg[k, ca.shape[0]:] == 0).all()
    if which == "lattice":
        assert not ref[17, 119] and ref.sum() == ref.shape[0] * (ref.shape[0] - 1) - 2


def test_teaser_scaled_end_to_end_matches_host_path(device):
    from dpfm_amd import ops
    crops, _ = batch("ragged")
    nmax = max(c[0].shape[0] for c in crops)
    a, b, off = pack(crops, device)
    got = ops.teaser(a, b, off, nmax, threads=4, estimate_scaling=True)
    scale, _ = ops.teaser_scale(a, b, off, nmax, BETA)
    adj, deg = ops.teaser_graph(a, b, off, nmax, BETA, scale=scale)
    ref = ops.teaser_solve_host(a.cpu().numpy(), b.cpu().numpy(), off.cpu().numpy(), nmax, adj.cpu().numpy(),
                                deg.cpu().numpy(), params(), threads=1, scale=scale.cpu().numpy())
    assert len(got) == 5
    for g, r in zip(got, ref + (scale.cpu().numpy(),)):
        np.testing.assert_array_equal(g, r)
    assert got[3][[0, 1, 5, 6], 0].all() and not got[3][[2, 3], 0].any()


def test_robust_registration_solver_upstream_defaults(device):
    from dpfm_amd.pose.teaser import RobustRegistrationSolver
    rng = np.random.default_rng(5)
    a, b, Tt, s = R.planted_scaled(rng, 300, 0.5, 1.7)
    p = RobustRegistrationSolver.Params()  # estimate_scaling = True, as upstream
    assert p.estimate_scaling
    p.noise_bound = 0.05
    solver = RobustRegistrationSolver(p, device=device)
    solver.solve(a.T, b.T)
    sol = solver.getSolution()
    assert sol.valid and abs(sol.scale - s) / s < 1e-3, sol.scale
    assert np.abs(sol.rotation - Tt[:3, :3]).max() < 5e-3 and np.abs(sol.translation - Tt[:3, 3]).max() < 0.05
    inl = np.linalg.norm(s * (a @ Tt[:3, :3].T) + Tt[:3, 3] - b, axis=1) < 0.06  # the planted inliers (noise 0.01)
    assert 100 < inl.sum() < 200
    M = sol.transform
    np.testing.assert_array_equal(M[3], [0, 0, 0, 1])
    assert np.linalg.norm(a[inl] @ M[:3, :3].T + M[:3, 3] - b[inl], axis=1).max() < 0.1


def test_default_path_unchanged(device):
    from dpfm_amd import ops
    rng = np.random.default_rng(3)
    crops = [planted(rng, n, f) for n, f in ((150, 0.8), (90, 0.3), (2, 1.0), (0, 1.0))]
    a, b, off = pack(crops, device)
    ref = run_host(crops, 150)
    for got in (ops.teaser(a, b, off, 150, threads=4), ops.teaser(a, b, off, 150, threads=4, estimate_scaling=False)):
        assert len(got) == 4
        for g, r in zip(got, ref):
            np.testing.assert_array_equal(g, r)
