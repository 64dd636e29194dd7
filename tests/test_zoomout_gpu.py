"""GPU: the ZoomOut kernels (csrc/zoomout.hip, ops.zoomout) against the fp64 loop of
tests/_zoomout_ref.py, piece by piece and end to end, on analytic eigenfunctions of a rectangle.

Index check. The device's point map may differ from the fp64 argmin only where two rows' scores lie
within the f32 evaluation's error of each other: the device's pick must score within tau_j of the
fp64 minimum, tau_j = c (k + 3) 2^-24 (max_i |E_i|^2 + max_i |E_i| |y_j|) with c derived from fp64
quantities of the inputs in _zoomout_ref.tau's docstring (the f32 rounding of E, of the row norm and
of the k-term dot product), never from device output. Such columns are capped at 3 % of n2 (the
reference alone has under 2 % of columns that near a tie: tests/test_zoomout_cpu.py).

Projection check. C[a, b] = sum_j m_j y_ja x_{p_j b} is evaluated as fmaf chains over the rows of a
64-row slab (the product m_j y_ja rounded once, then one rounding per term) and the slabs' partials
added in slab order, so to first order |C^ - C| <= (1 + min(n2, 64) + slabs - 1) u S <= (n2 + slabs)
2^-24 S with S = sum_j |m_j y_ja x_{p_j b}| (fp64) and slabs = ceil(n2 / 64); the kernel's C for
its own p is held to (n2 + slabs) 2^-24 S.
"""
import numpy as np
import pytest
import torch

import _zoomout_ref as R

pytestmark = pytest.mark.gpu

N1, N2 = 601, 333
SEEDS = (1, 2, 3, 4, 5)
SLAB = 64


@pytest.fixture(scope="module")
def cases():
    return {s: R.rect_case(s, N1, N2) for s in SEEDS}


@pytest.fixture(scope="module")
def naive_err(cases):
    return {s: R.map_error(c, R.point_map(c["ex"], c["ey"], c["C0"], N1, N2, 30)) for s, c in cases.items()}


@pytest.fixture(scope="module")
def ref_e2e(cases):
    """the fp64 loop at step 5, k_final 64, once per seed"""
    return {s: R.zoomout(c["ex"], c["ey"], c["mass"], c["C0"], N1, N2, 64, 5) for s, c in cases.items()}


def batch(crops, V1=None, V2=None, fill=None):
    """crops: list of (ex [n1, 64], ey [n2, 64], mass [n2], C0) -> padded host arrays + counts.
    fill(b, ex_pad, ey_pad, mass_pad, n1, n2) may write the padding."""
    B = len(crops)
    V1 = V1 or max(len(c[0]) for c in crops)
    V2 = V2 or max(len(c[1]) for c in crops)
    ex = np.zeros((B, V1, 64), np.float32)
    ey = np.zeros((B, V2, 64), np.float32)
    mass = np.zeros((B, V2), np.float32)
    C0 = np.stack([c[3] for c in crops]).astype(np.float32)
    n1 = np.array([len(c[0]) for c in crops], np.int32)
    n2 = np.array([len(c[1]) for c in crops], np.int32)
    for b, (x, y, m, _) in enumerate(crops):
        ex[b, :len(x)], ey[b, :len(y)], mass[b, :len(y)] = x, y, m
        if fill is not None:
            fill(b, ex[b], ey[b], mass[b], len(x), len(y))
    return ex, ey, mass, C0, n1, n2


def run(device, arrs, k_final=64, step=1, work=None):
    from dpfm_amd import ops
    ex, ey, mass, C0, n1, n2 = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrs)
    C, p = ops.zoomout(ex, ey, mass, C0, n1, n2, k_final=k_final, step=step, work=work)
    torch.cuda.synchronize()
    return C.cpu().numpy(), p.cpu().numpy()


def one(c, n1=N1, n2=N2):
    return (c["ex"][:n1], c["ey"][:n2], c["mass"][:n2], c["C0"])


def check_index(ex, ey, C, p_dev, n1, n2, k, cap=0.03):
    """p_dev against the fp64 argmin under C; returns the share of differing columns."""
    s = R.scores(ex, ey, C, n1, n2, k)
    p_ref = s.argmin(0)
    assert p_dev.min() >= 0 and p_dev.max() < n1
    diff = np.nonzero(p_dev != p_ref)[0]
    t = R.tau(ex, ey, C, n1, n2, k)
    over = s[p_dev[diff], diff] - s[p_ref[diff], diff]
    print(f"k {k}: {len(diff)} of {n2} columns differ; worst excess / tau "
          f"{(over / t[diff]).max() if len(diff) else 0:.3f}")
    assert np.all(over <= t[diff]), (k, float((over / t[diff]).max()))
    assert len(diff) <= cap * n2, (k, len(diff))
    return len(diff) / max(n2, 1)


def check_projection(ex, ey, mass, p, C_dev, n2, k):
    ex64, ey64, m64 = (np.asarray(a, np.float64) for a in (ex, ey, mass))
    want = R.project(ex, ey, mass, p, n2, k)
    S = (np.abs(ey64[:n2, :k]) * m64[:n2, None]).T @ np.abs(ex64[p[:n2], :k])
    bound = (n2 + -(-n2 // SLAB)) * R.U32 * S
    err = np.abs(C_dev.astype(np.float64) - want)
    print(f"k {k}: projection worst error / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert C_dev.shape == (k, k)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("k", [30, 31, 33, 37, 60, 64])
def test_one_iteration_per_piece(device, cases, k):
    """One jump 30 -> k: the projection onto k x k for the device's own 30-wide point map, then the
    nearest-neighbour pass at k under the device's own C."""
    c = cases[1]
    arrs = batch([one(c)])
    C30, p30 = run(device, arrs, k_final=30)
    assert np.array_equal(C30[0], c["C0"])
    if k == 30:
        check_index(c["ex"], c["ey"], c["C0"], p30[0], N1, N2, 30)
        return
    Ck, pk = run(device, arrs, k_final=k, step=k - 30)
    check_projection(c["ex"], c["ey"], c["mass"], p30[0], Ck[0], N2, k)
    check_index(c["ex"], c["ey"], Ck[0], pk[0], N1, N2, k)


def test_edges_in_one_ragged_batch(device, cases):
    """Every (n1, n2) of {1, 15, 16, 17, 601} x {0, 1, 16, 17, 333} in one batch padded to 608 / 336.
    The padded X rows are Y rows (signs undone): they would win the argmin if n1 were ignored; the
    padded Y rows and masses are large: they would wreck C if n2 were ignored."""
    c = cases[2]
    V1, V2 = 608, 336
    combos = [(a, b) for a in (1, 15, 16, 17, 601) for b in (0, 1, 16, 17, 333)]

    def fill(b, exp, eyp, mp, n1, n2):
        rows = np.arange(V1 - n1) % N2
        exp[n1:] = c["ey"][rows] * c["s"][None].astype(np.float32)
        eyp[n2:] = 1e3
        mp[n2:] = 1e3

    arrs = batch([one(c, a, b) for a, b in combos], V1, V2, fill)
    # the trap is live: with the counts ignored, padded X rows win columns of the fp64 argmin
    trap = R.point_map(arrs[0][0], c["ey"], c["C0"], V1, N2, 30)
    assert (trap >= 1).mean() > 0.5
    C, p = run(device, arrs, k_final=64, step=5)
    assert np.all(np.isfinite(C))
    for b, (n1, n2) in enumerate(combos):
        assert np.all(p[b, n2:] == 0), (n1, n2)
        assert p[b].min() >= 0 and p[b].max() < n1, (n1, n2)
        if n2 == 0:
            assert np.all(C[b] == 0), n1
            continue
        # the padding changes nothing: the crop alone, unpadded, gives the same bits
        Ca, pa = run(device, batch([one(c, n1, n2)]), k_final=64, step=5)
        assert np.array_equal(pa[0], p[b, :n2]), (n1, n2)
        assert np.array_equal(Ca[0], C[b]), (n1, n2)
        if n1 == 1:
            assert np.all(p[b] == 0)


@pytest.mark.parametrize("k_final", [30, 47, 64])
@pytest.mark.parametrize("step", [1, 5, 34])
def test_schedules(device, cases, step, k_final):
    """A short last step, a single jump, sizes that are no multiple of 4: the final point map
    against the fp64 loop's, the final C against the fp64 projection of the device's own previous
    point map (the same schedule stopped one size earlier)."""
    from dpfm_amd import ops
    c = cases[3]
    ks = R.schedule(k_final, step)
    assert ops.zoomout_schedule(k_final, step) == ks
    arrs = batch([one(c)])
    C, p = run(device, arrs, k_final=k_final, step=step)
    C_ref, p_ref = R.zoomout(c["ex"], c["ey"], c["mass"], c["C0"], N1, N2, k_final, step)
    assert C.shape == (1, k_final, k_final) and p.shape == (1, N2)
    differ = int((p[0] != p_ref).sum())
    print(f"step {step} k_final {k_final}: {differ} of {N2} columns differ from the fp64 loop")
    assert differ <= 0.01 * N2
    if len(ks) > 1:
        _, p_prev = run(device, arrs, k_final=ks[-2], step=step)
        check_projection(c["ex"], c["ey"], c["mass"], p_prev[0], C[0], N2, k_final)
        check_index(c["ex"], c["ey"], C[0], p[0], N1, N2, k_final)
    else:
        assert np.array_equal(C[0], c["C0"])


def test_scratch_contents_and_repeats_do_not_matter(device, cases):
    from dpfm_amd import _lib, ops
    arrs = batch([one(cases[s]) for s in SEEDS])
    nbytes = int(_lib.lib().pk_zoomout_work_size(len(SEEDS), N1, N2, 64, 5))
    assert nbytes > 0
    outs = []
    for fillv in (0xFF, 0x00):
        work = torch.full((nbytes,), fillv, dtype=torch.uint8, device=device)
        outs.append(run(device, arrs, 64, 5, work=work))
    outs.append(run(device, arrs, 64, 5))
    outs.append(run(device, arrs, 64, 5))
    for C, p in outs[1:]:
        assert np.array_equal(C, outs[0][0]) and np.array_equal(p, outs[0][1])
    with pytest.raises(_lib.PoseKernError):
        ops.zoomout(*(torch.from_numpy(a).to(device) for a in arrs), k_final=64, step=5,
                    work=torch.empty(nbytes - 1, dtype=torch.uint8, device=device))


def test_crop_alone_equals_crop_in_batch(device, cases):
    """96 crops (one row part per block) against the same crops alone (row parts merged by the second
    launch) and in a batch of 5: the same bits."""
    crops = [one(cases[SEEDS[b % 5]], N1 - 7 * (b % 3), N2 - 5 * (b % 4)) for b in range(96)]
    Cb, pb = run(device, batch(crops, N1, N2), 64, 5)
    C5, p5 = run(device, batch(crops[:5], N1, N2), 64, 5)
    assert np.array_equal(C5, Cb[:5]) and np.array_equal(p5, pb[:5])
    for b in (0, 7, 95):
        Ca, pa = run(device, batch([crops[b]], N1, N2), 64, 5)
        assert np.array_equal(Ca[0], Cb[b]) and np.array_equal(pa[0], pb[b]), b


def test_end_to_end_against_the_fp64_loop(device, cases, ref_e2e, naive_err):
    C, p = run(device, batch([one(cases[s]) for s in SEEDS]), 64, 5)
    for b, s in enumerate(SEEDS):
        C_ref, p_ref = ref_e2e[s]
        differ = int((p[b] != p_ref).sum())
        err = R.map_error(cases[s], p[b])
        print(f"seed {s}: {differ} of {N2} columns differ; map error {err:.4f} vs naive {naive_err[s]:.4f} "
              f"(ratio {err / naive_err[s]:.3f}); max |C - C_ref| {np.abs(C[b] - C_ref).max():.2e}")
        assert differ <= 0.01 * N2, s
        assert err <= 0.85 * naive_err[s], s


def test_solvers_agree_with_the_op(device, cases):
    from dpfm_amd import fmap2pointmap_solvers as S
    c = cases[4]
    C, p = run(device, batch([one(c)]), 64, 5)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    ex, ey, mass, C0 = t(c["ex"]), t(c["ey"]), t(c["mass"]), t(c["C0"])
    assert np.array_equal(S.zoomout_refine(C0, ex, ey, mass, k_final=64, step=5).cpu().numpy(), C[0])
    pm = S.zoomout_fmap2pointmap(C0[None], ex, ey, mass, k_final=64, step=5)
    assert pm.shape == (2, N2) and pm.dtype == torch.int64
    assert np.array_equal(pm[0].cpu().numpy(), p[0]) and np.array_equal(pm[1].cpu().numpy(), np.arange(N2))
    # the rectangle as a flat surface in space: the filter sees the refined one-per-point map
    CAD = t(np.concatenate([c["X"], np.zeros((N1, 1))], 1).astype(np.float32))
    PC = t(np.concatenate([c["Y"], np.zeros((N2, 1))], 1).astype(np.float32))
    diam = float(np.hypot(1.0, R.H))
    kept = S.zoomout_spacial_filtering_fmap2pointmap(C0, ex, ey, mass, CAD, PC, diam, k_final=64, step=5)
    want = S.spacial_filtering(CAD, PC, pm, diam)
    assert torch.equal(kept, want) and 0 < kept.shape[1] <= N2
    assert S.choose_fmap2pointmap_solver() is S.spacial_filtering_fmap2pointmap


def test_bad_arguments_raise(device, cases):
    from dpfm_amd import _lib, ops
    from dpfm_amd.pipeline import InferStep
    arrs = batch([one(cases[1], 64, 32)])
    dv = [torch.from_numpy(a).to(device) for a in arrs]
    for kw in (dict(k_final=29), dict(k_final=65), dict(step=0), dict(step=-3)):
        with pytest.raises(_lib.PoseKernError):
            ops.zoomout(*dv, **kw)
    with pytest.raises(_lib.PoseKernError):  # wider than the evecs
        ops.zoomout(dv[0][..., :40].contiguous(), dv[1], *dv[2:], k_final=41)
    with pytest.raises(_lib.PoseKernError):  # host tensors
        ops.zoomout(*(torch.from_numpy(a) for a in arrs))
    assert _lib.lib().pk_zoomout_work_size(1, 64, 32, 65, 1) == -1
    assert _lib.lib().pk_zoomout_work_size(1, 64, 32, 64, 0) == -1
    with pytest.raises(ValueError):
        InferStep(None, zoomout=(65, 1))
    C, p = ops.zoomout(dv[0][..., :40].contiguous(), dv[1][..., :47].contiguous(), *dv[2:], k_final=40, step=4)
    Cw, pw = ops.zoomout(*dv, k_final=40, step=4)  # columns past k_final are never read
    assert torch.equal(C, Cw) and torch.equal(p, pw)


@pytest.fixture(scope="module")
def infer_setup(device):
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import make_frame_batch
    torch.manual_seed(0)
    F, N = 2, 256
    fb, op = make_frame_batch(F, N, N, seed=71, device=device)
    return fb, op, DPFMNet().to(device).eval(), N


def test_infer_step_default_is_unchanged(device, infer_setup):
    from dpfm_amd.dataset.object import CropFormation
    from dpfm_amd.pipeline import InferStep
    fb, op, model, N = infer_setup
    crops = CropFormation(n1=N, npoint=N, seed=3)(fb)
    plain = InferStep(model, hypotheses=256)(fb, op, crops)
    off = InferStep(model, hypotheses=256, zoomout=None)(fb, op, crops)
    torch.cuda.synchronize()
    assert set(plain) == set(off) and "C_zo" not in off
    assert plain["cand"].shape[1] == 5 * N
    for key, v in plain.items():
        if torch.is_tensor(v):
            w = off[key]
            if key == "corres":  # (its last row is the spill row of the invalid slots: unspecified)
                v, w = v[:-1], w[:-1]
            assert torch.equal(v, w), key


def test_infer_step_zoomout_eager_graphed_pipelined(device, infer_setup):
    """InferStep(zoomout=(64, 5)): one refined candidate per crop point, C_zo in the outputs; the
    captured step replays bit-equal to the eager call, and so does the three-stage pipeline."""
    from dpfm_amd import ops
    from dpfm_amd.dataset.object import CropFormation
    from dpfm_amd.pipeline import GraphedInfer, InferStep, PipelinedInfer, _counts, zoomout_p2p_batched
    fb, op, model, N = infer_setup
    B = op.cad_evecs.shape[0]
    crops = CropFormation(n1=N, npoint=N, seed=3)(fb)
    eager = InferStep(model, hypotheses=256, zoomout=(64, 5))(fb, op, crops)
    torch.cuda.synchronize()
    assert eager["C_zo"].shape == (B, 64, 64) and eager["cand"].shape == (B, N, 2)
    n1, n2 = _counts(op.cad_n, B, N, device), _counts(crops.n2, B, N, device)
    C, p = ops.zoomout(op.cad_evecs, op.pc_evecs, op.pc_mass, eager["C"], n1, n2, k_final=64, step=5)
    assert torch.equal(C, eager["C_zo"]) and torch.equal(p, eager["cand"][..., 0])
    assert torch.equal(eager["cand"][..., 1], torch.arange(N, device=device)[None].expand(B, N))
    Cb, pb = zoomout_p2p_batched(eager["C"], op.cad_evecs, op.pc_evecs, op.pc_mass, n1, n2, 64, 5)
    assert torch.equal(Cb, C) and torch.equal(pb[:, 0], p) and pb.shape == (B, 2, N)
    assert int(eager["n_corr"].max()) <= N
    ref = {k: v.clone() for k, v in eager.items() if torch.is_tensor(v)}
    keys = ("C", "C_zo", "cand", "p_pred", "n_corr", "ir", "T", "metrics")
    g = GraphedInfer(CropFormation(n1=N, npoint=N, seed=3), InferStep(model, hypotheses=256, zoomout=(64, 5)), fb, op)
    for _ in range(2):
        out = g()
        torch.cuda.synchronize()
        for key in keys:
            assert torch.equal(out[key], ref[key]), key
    pl = PipelinedInfer(CropFormation(n1=N, npoint=N, seed=3), InferStep(model, hypotheses=256, zoomout=(64, 5)), fb,
                        op, stages=3)
    assert pl() is None
    outs = [pl() for _ in range(3)] + [pl.flush()]
    torch.cuda.synchronize()
    for out in outs[-3:]:
        for key in keys:
            assert torch.equal(out[key], ref[key]), key
