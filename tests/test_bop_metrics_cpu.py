"""BOP pose errors, CPU part: the symmetry sets of dataset/formats.py against tests/_bop_ref.py,
object_frame(symmetries=True), the reference's own self-checks, the recall helpers, the ctypes
table entry, and — on the reference alone — that the seeded GPU cases separate every crop's best
symmetry from the runner-up (so test_bop_metrics_gpu.py may compare `best` exactly)."""
import json
import os
import re

import numpy as np
import pytest

import _bop_cases as C
import _bop_ref as R
from dpfm_amd.dataset import formats as FMT

DISC = [-1, 0, 0, 4.0, 0, -1, 0, -6.0, 0, 0, 1, 0, 0, 0, 0, 1]  # half turn about the z axis through (2, -3) mm
CONT = {"axis": [0, 0, 1], "offset": [20.0, -30.0, 5.0]}
INFOS = [({"diameter": 100.0}, 1),
         ({"diameter": 100.0, "symmetries_discrete": [DISC]}, 2),
         ({"diameter": 100.0, "symmetries_continuous": [CONT]}, 315),
         ({"diameter": 100.0, "symmetries_discrete": [DISC], "symmetries_continuous": [CONT]}, 630)]


@pytest.mark.parametrize("info,count", INFOS, ids=["none", "discrete", "continuous", "both"])
def test_symmetry_transformations_match_reference(info, count):
    got = FMT.symmetry_transformations(info)
    ref = R.symmetry_transformations(info)
    assert got.shape == (count, 4, 4) and got.dtype == np.float64 and ref.shape == got.shape
    # rotations of unit size, translations of a few cm: a handful of roundings each
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13)
    assert np.array_equal(got[0], np.eye(4)), "element 0 is exactly the identity"
    for T in got:
        Rm = T[:3, :3]
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-14 and np.linalg.det(Rm) > 0
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def test_symmetry_translations_are_scaled():
    info = INFOS[3][0]
    mm = FMT.symmetry_transformations(info, scale=1.0)
    cm = FMT.symmetry_transformations(info)
    np.testing.assert_array_equal(cm[:, :3, :3], mm[:, :3, :3])
    np.testing.assert_allclose(cm[:, :3, 3], 0.1 * mm[:, :3, 3], rtol=1e-15, atol=0)
    assert np.abs(mm[:, :3, 3]).max() > 10.0  # the offset axis does move points
    # a coarser step: n = ceil(pi / step) rotations
    assert FMT.symmetry_transformations(INFOS[2][0], max_sym_disc_step=0.5).shape[0] == 7
    # the continuous set turns about the axis through the offset: the offset point is fixed
    fixed = np.array([2.0, -3.0, 0.5])
    for T in cm[:315:37]:
        np.testing.assert_allclose(R.transform(T, fixed[None])[0], fixed, rtol=0, atol=1e-14)


def test_object_frame_symmetries(tmp_path):
    from test_formats_cpu import GOLD, _write_bop
    g = np.load(os.path.join(GOLD, "lm_frame.npz"))
    poses = [(np.eye(3), np.array([0.0, 0.0, 80.0]), 1 + (j % 2)) for j in range(g["masks"].shape[0])]
    _, models = _write_bop(tmp_path, g, poses)
    rng = np.random.default_rng(0)
    for oid in (1, 2):
        FMT.write_ply(models / f"obj_{oid:06d}.ply", rng.normal(size=(50, 3)) * 40)
    infos = {"1": INFOS[1][0], "2": INFOS[0][0]}
    (models / "models_info.json").write_text(json.dumps(infos))
    sc = FMT.BopScenes(tmp_path, "train_pbr")
    plain = FMT.object_frame(sc, 0, 0, models, cad_cache={})
    assert set(plain) == {"depth", "mask", "K", "depth_scale", "R_m2c", "t_m2c", "obj_id", "visib_fract", "cad",
                          "diam_cad", "rgb"}
    with_s = FMT.object_frame(sc, 0, 0, models, cad_cache={}, symmetries=True)
    assert set(with_s) == set(plain) | {"syms"}
    np.testing.assert_array_equal(with_s["syms"], FMT.symmetry_transformations(infos["1"]))
    assert with_s["syms"].shape == (2, 4, 4)
    assert FMT.object_frame(sc, 0, 1, models, cad_cache={}, symmetries=True)["syms"].shape == (1, 4, 4)


def test_reference_self_checks():
    rng = np.random.default_rng(1)
    half = np.diag([-1.0, -1.0, 1.0, 1.0])
    base = rng.normal(size=(60, 3)) * 6
    pts = np.concatenate([base, R.transform(half, base)], 0)  # closed under the half turn about z
    Tg = C.gt_pose(rng)
    Te = Tg @ half
    syms = np.stack([np.eye(4), half])
    e = R.errors(Te, Tg, C.lm_K(), pts, syms)
    assert e["mssd"] <= 1e-12 and e["adi"] <= 1e-12 and e["best"][0] == 1
    assert R.add(Te, Tg, pts) > 1.0
    # one symmetry: MSSD is the largest vertex distance
    Te2 = Tg @ C.pose(rng, 5.0, 1.0)
    d = np.linalg.norm(R.transform(Te2, pts) - R.transform(Tg, pts), axis=1)
    assert R.mssd_all(Te2, Tg, pts, np.eye(4)[None]).min() == d.max()
    # ADI never exceeds ADD, and is 0 for equal poses
    assert R.adi(Te2, Tg, pts) <= R.add(Te2, Tg, pts) and R.adi(Tg, Tg, pts) == 0.0


def test_bop_recall_hand_values():
    from dpfm_amd.pose.metrics import bop_average_recall, bop_recall
    err = [0.5, 1.5, 2.5, float("nan")]
    # thresholds 1, 2, 3 -> 1/4, 2/4, 3/4 below (strict; the NaN never counts)
    assert bop_recall(err, [1.0, 2.0, 3.0]) == pytest.approx(0.5, abs=1e-15)
    assert bop_recall([1.0], [1.0]) == 0.0
    # MSSD: diameter 10 -> thresholds 0.5, 1.0, ..., 5.0; error 1.2 is below 8 of them, 10.0 below none
    # MSPD: width 1280 -> r = 2, thresholds 10, 20, ..., 100; 35 px is below 7, 5 px below all 10
    ar = bop_average_recall([1.2, 10.0], [35.0, 5.0], 10.0, 1280)
    assert ar == pytest.approx(0.5 * ((8 + 0) / 20 + (7 + 10) / 20), abs=1e-15)
    # one diameter per estimate: 1.2 against diameter 4 (0.2 ... 2.0) is below 4; 10 against 100 (5 ... 50) below 9
    ar = bop_average_recall([1.2, 10.0], [35.0, 5.0], [4.0, 100.0], 640)
    assert ar == pytest.approx(0.5 * ((4 + 9) / 20 + (3 + 9) / 20), abs=1e-15)


def test_entry_point_table_and_tiling_constants():
    from dpfm_amd import _lib, ops
    P, I = _lib._P, _lib._I
    assert _lib.SIGNATURES["pk_bop_errors"] == [P, P, I, I, P, P, P, P, P, I, P, P, P, P]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "posekern.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define PK_BOP_(\w+) (\d+)", hdr)}
    assert defs == {"QUERY_BLOCK": C.QUERY_BLOCK, "TARGET_TILE": C.TARGET_TILE, "SYM_CHUNK": C.SYM_CHUNK}
    assert (ops.BOP_QUERY_BLOCK, ops.BOP_TARGET_TILE, ops.BOP_SYM_CHUNK) == (C.QUERY_BLOCK, C.TARGET_TILE, C.SYM_CHUNK)
    assert ops.bop_errors_work_len(3, 100, 0) == 3 * 402 and ops.bop_errors_work_len(2, 10, 630) == 2 * 1300


def test_frame_batch_symmetry_fields_are_optional():
    """FrameBatch.syms / sym_off / smax are defaulted: existing constructors keep working."""
    from dpfm_amd.dataset.object import FrameBatch
    import dataclasses
    f = {x.name: x for x in dataclasses.fields(FrameBatch)}
    assert f["syms"].default is None and f["sym_off"].default is None and f["smax"].default == 0


def test_seeded_gpu_cases_separate_their_best_symmetry():
    """On the reference alone: in every crop of the GPU tests' symmetry batch the best MSSD / MSPD
    symmetry beats the runner-up by more than 100 x the comparison tolerance (the duplicate pair of
    DUP_CROP counted once), the last-index and duplicate crops are what they claim, and the ADI batch
    (one symmetry each) has nothing to separate."""
    crops, K, refs = C.sym_batch()
    assert [len(c["syms"]) for c in crops[:len(C.SYM_COUNTS)]] == C.SYM_COUNTS
    for k, (c, r) in enumerate(zip(crops, refs)):
        dup = (2, 3) if k == C.DUP_CROP else None
        m3, m2 = C.best_margins(r, dup)
        assert m3 > 100 * C.tol(r["scale3"], r["mssd"]), (k, m3)
        assert m2 > 100 * C.tol(r["scale2"], r["mspd"]), (k, m2)
    last = refs[C.LAST_CROP]
    assert last["best"][0] == len(crops[C.LAST_CROP]["syms"]) - 1
    dupr = refs[C.DUP_CROP]
    assert dupr["best"] == (2, 2) and dupr["all3"][2] == dupr["all3"][3] and dupr["all2"][2] == dupr["all2"][3]
    assert len({r["best"][0] for r in refs}) > 3  # the best symmetry is not trivially 0
    for r in C.adi_batch()[2]:
        assert r["best"] == (0, 0) and len(r["all3"]) == 1
