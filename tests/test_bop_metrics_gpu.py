"""BOP pose errors on the device (pk_bop_errors / ops.bop_errors) against the naive numpy fp64
restatement tests/_bop_ref.py, on the seeded cases of tests/_bop_cases.py.

Tolerance (derived, not measured): |got - ref| <= 1e-12 * scale + 1e-12 * |ref|, scale the largest
absolute coordinate of the transformed points (MSSD, ADI) or the largest pixel coordinate (MSPD):
about 20 fp64 roundings on numbers of that size per term — the difference of two nearby points
cancels, so the error is absolute — plus n 2^-53 <= 6e-13 relative for ADI's mean; an FMA instead
of a separately rounded product and sum stays inside the same bound."""
import dataclasses

import numpy as np
import pytest
import torch

import _bop_cases as C

pytestmark = pytest.mark.gpu


def _dev(p, device, K=None):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    d = dict(cad=t(p["cad"]), off=t(p["off"]), T_est=t(p["T_est"]), T_gt=t(p["T_gt"]), sym=t(p["sym"]),
             sym_off=t(p["sym_off"]), smax=p["smax"])
    if K is not None:
        d["K"] = t(np.broadcast_to(K, (len(p["T_est"]), 3, 3)))
    return d


def _run(d, nmax, K=True, sym=True):
    from dpfm_amd import ops
    out, best = ops.bop_errors(d["cad"], d["off"], nmax, d["T_est"], d["T_gt"], d["K"] if K else None,
                               d["sym"] if sym else None, d["sym_off"] if sym else None, d["smax"] if sym else None)
    return out.cpu().numpy(), best.cpu().numpy()


def _check_row(got, ref, what):
    for col, key, sk in ((0, "mssd", "scale3"), (1, "mspd", "scale2"), (2, "adi", "scale3")):
        err, bound = abs(got[col] - ref[key]), C.tol(ref[sk], ref[key])
        print(f"{what} {key}: got {got[col]:.17g} ref {ref[key]:.17g} |diff| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (what, key, err, bound)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_adi_ragged_sizes_against_reference(device):
    """V in {1, 63, 64, 65, 255, 256, 257}, the query block +- 1, the LDS target tile +- 1 and a
    crop with exact duplicate targets, in one batch with nmax above the largest; twice: bit-identical."""
    crops, K, refs = C.adi_batch()
    d = _dev(C.pack(crops), device, K)
    out, best = _run(d, C.ADI_NMAX)
    for b, r in enumerate(refs):
        _check_row(out[b], r, f"crop {b} V={len(crops[b]['pts'])}")
    assert (best == 0).all()
    out2, best2 = _run(d, C.ADI_NMAX)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(best, best2)
    # the identity-only default equals the explicit identity set, bit for bit
    out3, best3 = _run(d, C.ADI_NMAX, sym=False)
    assert np.array_equal(_bits(out), _bits(out3)) and np.array_equal(best, best3)
    # no K: the MSPD column is NaN, its best -1, the rest unchanged
    out4, best4 = _run(d, C.ADI_NMAX, K=False)
    assert np.isnan(out4[:, 1]).all() and (best4[:, 1] == -1).all()
    assert np.array_equal(_bits(out4[:, [0, 2]]), _bits(out[:, [0, 2]])) and np.array_equal(best4[:, 0], best[:, 0])


def test_symmetry_counts_ragged_against_reference(device):
    """S in {1, 2, 64, 65, 630}, the symmetry chunk +- 1, a crop whose best symmetry is the last
    index and a crop with two identical symmetries (the lower index wins), in one batch."""
    crops, K, refs = C.sym_batch()
    p = C.pack(crops)
    d = _dev(p, device, K)
    nmax = max(len(c["pts"]) for c in crops) + 3
    out, best = _run(d, nmax)
    for b, r in enumerate(refs):
        _check_row(out[b], r, f"crop {b} S={len(crops[b]['syms'])}")
        # every crop separates its best from the runner-up by > 100 x the tolerance (asserted on the
        # reference alone in test_bop_metrics_cpu.py), so the index is comparable exactly
        assert tuple(best[b]) == r["best"], (b, best[b], r["best"])
    assert best[C.LAST_CROP, 0] == len(crops[C.LAST_CROP]["syms"]) - 1
    assert tuple(best[C.DUP_CROP]) == (2, 2)
    out2, best2 = _run(d, nmax)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(best, best2)
    # the default smax (the total symmetry count: always enough) gives the same result
    d2 = dict(d, smax=None)
    out3, best3 = _run(d2, nmax)
    assert np.array_equal(_bits(out), _bits(out3)) and np.array_equal(best, best3)


def test_pose_correct_up_to_a_symmetry(device):
    """Reference-free: T_est = T_gt S_k on a cloud closed under S_k scores ~0 MSSD / MSPD / ADI with
    best = k, while the symmetry-blind ADD of pk_pose_metrics calls it a failure."""
    from dpfm_amd import ops
    crops, K = C.closed_batch()
    d = _dev(C.pack(crops), device, K)
    nmax = max(len(c["pts"]) for c in crops)
    out, best = _run(d, nmax)
    add = ops.pose_metrics(d["cad"], d["off"], nmax, d["T_est"], d["T_gt"]).cpu().numpy()[:, 0]
    for b, c in enumerate(crops):
        scale3 = np.abs(c["pts"] @ c["T_gt"][:3, :3].T + c["T_gt"][:3, 3]).max()
        print(f"crop {b}: k {c['k']} out {out[b]} best {best[b]} ADD {add[b]}")
        assert out[b, 0] <= C.tol(scale3, 0.0) and out[b, 2] <= C.tol(scale3, 0.0)
        assert out[b, 1] <= C.tol(640.0, 0.0)
        assert tuple(best[b]) == (c["k"], c["k"])
        assert add[b] > 1.0


def test_unevaluated_crops_and_guards(device):
    """NaN / inf in T_est, a 0-point crop and a crop over nmax give a NaN row and best (-1, -1);
    the other crops equal the reference; sentinel guard rows around out, best and work stay
    untouched (the entry point is called directly on caller-allocated buffers)."""
    from dpfm_amd import _lib, ops
    from dpfm_amd._lib import ptr
    src, K, refs = C.sym_batch()
    rng = np.random.default_rng(9)
    crops = [dict(c) for c in (src[1], src[2], src[5], src[6], src[7], src[0])]
    crops[1]["T_est"] = crops[1]["T_est"].copy()
    crops[1]["T_est"][1, 2] = np.nan
    crops[2]["T_est"] = crops[2]["T_est"].copy()
    crops[2]["T_est"][0, 3] = np.inf
    crops[3]["pts"] = np.zeros((0, 3))
    crops[4]["pts"] = rng.normal(size=(400, 3)) * 6.0
    ref = {0: refs[1], 5: refs[0]}
    nmax = 300  # crops 0, 1, 2, 5 fit (<= 175 points); crop 4 does not
    assert all(len(crops[b]["pts"]) <= nmax for b in (0, 1, 2, 5)) and len(crops[4]["pts"]) > nmax
    p = C.pack(crops)
    d = _dev(p, device, K)
    B, smax = len(crops), p["smax"]
    out, best = _run(d, nmax)
    for b in range(B):
        if b in ref:
            _check_row(out[b], ref[b], f"crop {b}")
            assert tuple(best[b]) == ref[b]["best"]
        else:
            assert np.isnan(out[b]).all() and tuple(best[b]) == (-1, -1), (b, out[b], best[b])

    G, SENT = 2, -777.25
    wl = ops.bop_errors_work_len(B, nmax, smax)
    out_g = torch.full((B + 2 * G, 3), SENT, dtype=torch.float64, device=device)
    best_g = torch.full((B + 2 * G, 2), -777, dtype=torch.int32, device=device)
    work_g = torch.full((wl + 2 * 64,), SENT, dtype=torch.float64, device=device)
    _lib.call("pk_bop_errors", ptr(d["cad"]), ptr(d["off"]), B, nmax, ptr(d["T_est"]), ptr(d["T_gt"]), ptr(d["K"]),
              ptr(d["sym"]), ptr(d["sym_off"]), smax, ptr(work_g[64:64 + wl]), ptr(out_g[G:G + B]),
              ptr(best_g[G:G + B]), _lib.stream(device))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out_g[G:G + B].cpu().numpy()), _bits(out))
    assert np.array_equal(best_g[G:G + B].cpu().numpy(), best)
    for t, s in ((out_g[:G], SENT), (out_g[G + B:], SENT), (best_g[:G], -777), (best_g[G + B:], -777),
                 (work_g[:64], SENT), (work_g[64 + wl:], SENT)):
        assert bool((t == s).all())
    # B = 0 and nmax = 0 return OK and touch nothing
    _lib.call("pk_bop_errors", None, None, 0, nmax, None, None, None, None, None, 0, None, None, None,
              _lib.stream(device))
    out_g.fill_(SENT)
    _lib.call("pk_bop_errors", ptr(d["cad"]), ptr(d["off"]), B, 0, ptr(d["T_est"]), ptr(d["T_gt"]), ptr(d["K"]),
              ptr(d["sym"]), ptr(d["sym_off"]), smax, ptr(work_g), ptr(out_g[G:G + B]), ptr(best_g[G:G + B]),
              _lib.stream(device))
    torch.cuda.synchronize()
    assert bool((out_g == SENT).all())
    e = torch.zeros((0, 4, 4), dtype=torch.float64, device=device)
    o0, b0 = ops.bop_errors(d["cad"][:0], d["off"][:1], nmax, e, e)
    assert o0.shape == (0, 3) and b0.shape == (0, 2)
    with pytest.raises(_lib.PoseKernError):  # an invalid argument is an error, not a silent skip
        _lib.call("pk_bop_errors", ptr(d["cad"]), ptr(d["off"]), B, nmax, ptr(d["T_est"]), ptr(d["T_gt"]), None,
                  ptr(d["sym"]), None, smax, ptr(work_g), ptr(out_g), ptr(best_g), _lib.stream(device))


def test_single_crop_wrappers_equal_batched(device):
    """pose/metrics.py mssd / mspd / adi (bop_toolkit's names and signatures) on one crop return
    the batched call's numbers."""
    from dpfm_amd.pose import metrics as M
    crops, K, refs = C.sym_batch()
    p = C.pack(crops)
    d = _dev(p, device, K)
    out, _ = M.bop_errors_batched(d["cad"], d["off"], 300, d["T_est"], d["T_gt"], d["K"], d["sym"], d["sym_off"],
                                  d["smax"])
    out = out.cpu().numpy()
    for b in (1, 5, C.DUP_CROP):
        c = crops[b]
        syms = [{"R": S[:3, :3], "t": S[:3, 3].reshape(3, 1)} for S in c["syms"]]
        Re, te, Rg, tg = c["T_est"][:3, :3], c["T_est"][:3, 3:], c["T_gt"][:3, :3], c["T_gt"][:3, 3:]
        assert M.mssd(Re, te, Rg, tg, c["pts"], syms) == out[b, 0]
        assert M.mspd(Re, te, Rg, tg, K, c["pts"], syms) == out[b, 1]
        assert M.adi(Re, te, Rg, tg, c["pts"]) == out[b, 2]


def test_infer_step_bop_metrics(device):
    """InferStep(bop_metrics=True): `bop` equals ops.bop_errors on the returned T; every other key
    equals the default step's bit for bit; the default step has no `bop` key; one GraphedInfer
    capture and two replays give identical `bop`, and so do PipelinedInfer's two buffers."""
    from dpfm_amd import ops
    from dpfm_amd.dataset.object import CropFormation
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import GraphedInfer, InferStep, PipelinedInfer, make_frame_batch
    torch.manual_seed(0)
    F, N, E = 4, 512, 4
    fb, op = make_frame_batch(F, N, N, seed=71, device=device)
    sets = [np.eye(4)[None], C.cyclic_set(9, [0.0, 0.0, 1.0], np.zeros(3)), C.cyclic_set(2, [1.0, 0.0, 0.0], np.ones(3)),
            np.eye(4)[None]]
    fb = dataclasses.replace(fb, syms=torch.as_tensor(np.concatenate(sets), device=device),
                             sym_off=ops.packed_offsets([len(s) for s in sets], device), smax=9)
    model = DPFMNet().to(device).eval()
    crops = CropFormation(n1=N, npoint=N, seed=3)(fb)
    base = InferStep(model, hypotheses=256, icp_evaluations=E)(fb, op, crops)
    out = InferStep(model, hypotheses=256, icp_evaluations=E, bop_metrics=True)(fb, op, crops)
    assert not any(k.startswith("bop") for k in base)
    assert set(out) == set(base) | {"bop", "bop_best", "bop_icp"}
    for k, v in base.items():
        a, b = (v, out[k]) if v.dtype != torch.float64 else (v.view(torch.int64), out[k].view(torch.int64))
        if k == "corres":  # its last row is the spill row every invalid slot is scattered to: any of them may land
            a, b = a[:-1], b[:-1]
        assert torch.equal(a, b), k
    T_gt = torch.zeros((F, 4, 4), dtype=torch.float64, device=device)
    T_gt[:, :3, :3], T_gt[:, :3, 3], T_gt[:, 3, 3] = fb.R.view(F, 3, 3), fb.t, 1.0
    want, wbest = ops.bop_errors(fb.cad64, fb.cad_off, N, out["T"], T_gt, fb.K, fb.syms, fb.sym_off, 9)
    assert torch.equal(out["bop"], want) and torch.equal(out["bop_best"], wbest)
    assert torch.isfinite(out["bop"]).all() and torch.isfinite(out["bop_icp"]).all()
    assert torch.equal(out["bop_icp"], ops.bop_errors(fb.cad64, fb.cad_off, N, out["T_icp"], T_gt, fb.K, fb.syms,
                                                      fb.sym_off, 9)[0])
    g = GraphedInfer(CropFormation(n1=N, npoint=N, seed=3), InferStep(model, hypotheses=256, bop_metrics=True), fb, op)
    first = {k: g()[k].clone() for k in ("bop", "bop_best", "T")}
    again = {k: g()[k].clone() for k in ("bop", "bop_best", "T")}
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], out[k]), k
    p = PipelinedInfer(CropFormation(n1=N, npoint=N, seed=3), InferStep(model, hypotheses=256, bop_metrics=True), fb, op)
    for _ in range(3):  # both ping-pong buffers
        o = p()
        torch.cuda.synchronize()
        assert torch.equal(o["bop"], out["bop"]) and torch.equal(o["bop_best"], out["bop_best"])


def test_frame_batch_packs_symmetry_sets(device):
    """pipeline.frame_batch: a frame without "syms" gets the identity; none at all leaves the fields None."""
    from dpfm_amd.pipeline import frame_batch
    base = dict(depth=np.zeros((4, 6), np.uint16), mask=np.zeros((4, 6), np.uint8), K=np.eye(3), depth_scale=1.0,
                R_m2c=np.eye(3), t_m2c=np.zeros(3), cad=np.ones((5, 3)), diam_cad=10.0)
    plain = frame_batch([dict(base), dict(base)], device)
    assert plain.syms is None and plain.sym_off is None and plain.smax == 0
    s3 = C.cyclic_set(3, [0.0, 0.0, 1.0], np.ones(3))
    fb = frame_batch([dict(base), dict(base, syms=s3), dict(base)], device)
    assert fb.sym_off.tolist() == [0, 1, 4, 5] and fb.smax == 3 and fb.syms.dtype == torch.float64
    np.testing.assert_array_equal(fb.syms.cpu().numpy(), np.concatenate([np.eye(4)[None], s3, np.eye(4)[None]]))
