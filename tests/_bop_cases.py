"""Seeded inputs of the BOP pose-error tests and their reference values (tests/_bop_ref.py),
computed once per process and shared: test_bop_metrics_gpu.py compares the kernels against them,
test_bop_metrics_cpu.py checks on the reference alone that every crop's best symmetry is separated
from the runner-up by more than 100 x the tolerance, so that `best` can be compared exactly.

CAD-like clouds with coordinates of order 10 (cm), ground-truth poses in front of the LM camera
(tests/golden/lm_frame.npz K), estimates a few cm / degrees away."""
import functools
import os

import numpy as np

import _bop_ref as R

# pk_bop_errors' tiling (include/posekern.h PK_BOP_QUERY_BLOCK / PK_BOP_TARGET_TILE / PK_BOP_SYM_CHUNK;
# test_bop_metrics_cpu.py checks these three against the header and against dpfm_amd.ops)
QUERY_BLOCK, TARGET_TILE, SYM_CHUNK = 512, 1024, 8

ADI_SIZES = [1, 63, 64, 65, 255, 256, 257, QUERY_BLOCK - 1, QUERY_BLOCK, QUERY_BLOCK + 1,
             TARGET_TILE - 1, TARGET_TILE, TARGET_TILE + 1]
ADI_NMAX = TARGET_TILE + 76          # above the largest crop
SYM_COUNTS = [1, 2, 64, 65, 630, SYM_CHUNK - 1, SYM_CHUNK, SYM_CHUNK + 1]


def lm_K():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "lm_frame.npz"))["K"].astype(np.float64).reshape(3, 3)


def pose(rng, rot_deg, trans, centre=(0.0, 0.0, 0.0)):
    """A rigid 4x4: rotation of rot_deg about a random axis, translation centre + N(0, trans)."""
    axis = rng.normal(size=3)
    T = np.eye(4)
    T[:3, :3] = R.rotation(np.deg2rad(rot_deg), axis)
    T[:3, 3] = np.asarray(centre) + rng.normal(size=3) * trans
    return T


def gt_pose(rng):
    return pose(rng, rng.uniform(20, 160), 3.0, centre=(2.0, -3.0, 80.0))


def cyclic_set(S, axis, offset):
    """S rotations by 2 pi k / S about `axis` through `offset` (element 0 the identity)."""
    out = []
    for k in range(S):
        T = np.eye(4)
        T[:3, :3] = R.rotation(2.0 * np.pi * k / S, axis)
        T[:3, 3] = offset - T[:3, :3] @ offset
        out.append(T)
    return np.stack(out)


def tol(scale, ref):
    """The issue's derived bound: ~20 fp64 roundings on numbers of size `scale` (absolute: the
    difference of two nearby points cancels) plus the mean's n 2^-53 relative term."""
    return 1e-12 * scale + 1e-12 * abs(ref)


def pack(crops):
    """crops: list of dict(pts, T_est, T_gt, syms) -> packed numpy arrays."""
    n = [len(c["pts"]) for c in crops]
    s = [len(c["syms"]) for c in crops]
    return dict(cad=np.concatenate([c["pts"].reshape(-1, 3) for c in crops], 0),
                off=np.concatenate([[0], np.cumsum(n)]).astype(np.int64),
                T_est=np.stack([c["T_est"] for c in crops]), T_gt=np.stack([c["T_gt"] for c in crops]),
                sym=np.concatenate([c["syms"] for c in crops], 0),
                sym_off=np.concatenate([[0], np.cumsum(s)]).astype(np.int64), smax=max(s))


def reference(crops, K):
    return [R.errors(c["T_est"], c["T_gt"], K, c["pts"], c["syms"]) for c in crops]


@functools.lru_cache(maxsize=None)
def adi_batch():
    """Ragged ADI sizes in one batch (identity symmetry set); the last crop carries exact duplicate
    target points (its second half repeats its first)."""
    rng = np.random.default_rng(20261020)
    crops = []
    for n in ADI_SIZES + [300]:
        pts = rng.normal(size=(n, 3)) * 6.0
        if n == 300:
            pts[150:] = pts[:150]
        Tg = gt_pose(rng)
        crops.append(dict(pts=pts, T_gt=Tg, T_est=Tg @ pose(rng, 4.0, 1.5), syms=np.eye(4)[None]))
    K = lm_K()
    return crops, K, reference(crops, K)


DUP_CROP, LAST_CROP = len(SYM_COUNTS) + 1, len(SYM_COUNTS)


@functools.lru_cache(maxsize=None)
def sym_batch():
    """Ragged symmetry counts in one batch. Crop k < len(SYM_COUNTS) has SYM_COUNTS[k] symmetries
    (630: a models_info entry with one discrete and one continuous symmetry; the others a cyclic
    group about an offset axis) and an estimate near T_gt S_j for a seeded j. Crop LAST_CROP: 12
    symmetries, the estimate next to the last. Crop DUP_CROP: 5 symmetries of which 2 and 3 are the
    same matrix and the estimate sits next to it (the lower index must be reported)."""
    rng = np.random.default_rng(630)
    crops = []
    info630 = {"symmetries_discrete": [[-1, 0, 0, 0.4, 0, -1, 0, -0.6, 0, 0, 1, 0, 0, 0, 0, 1]],
               "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [2.0, -3.0, 0.0]}]}
    for k, S in enumerate(SYM_COUNTS + [12, 5]):
        n = 90 + 17 * k
        pts = rng.normal(size=(n, 3)) * 6.0
        if S == 630:
            syms = R.symmetry_transformations(info630)
        else:
            syms = cyclic_set(S, rng.normal(size=3), rng.normal(size=3))
        j = int(rng.integers(0, S))
        if k == LAST_CROP:
            j = S - 1
        if k == DUP_CROP:
            syms[3] = syms[2]
            j = 2
        Tg = gt_pose(rng)
        crops.append(dict(pts=pts, T_gt=Tg, T_est=Tg @ syms[j] @ pose(rng, 1.0, 0.3), syms=syms))
    K = lm_K()
    return crops, K, reference(crops, K)


def best_margins(ref, dup=None):
    """Per column (MSSD, MSPD): runner-up minus best of the per-symmetry list, the duplicate of
    the best left out for the crop built with one (inf for a single symmetry)."""
    out = []
    for key, b in (("all3", ref["best"][0]), ("all2", ref["best"][1])):
        v = np.array(ref[key], dtype=np.float64)
        skip = {b} | ({dup[0], dup[1]} if dup is not None and b in dup else set())
        rest = [x for i, x in enumerate(v) if i not in skip]
        out.append(min(rest) - v[b] if rest else np.inf)
    return out


@functools.lru_cache(maxsize=None)
def closed_batch():
    """Reference-free: clouds closed under the quarter turn about z (exact in fp64: the turn permutes
    and negates coordinates) and T_est = T_gt S_k for k = 1, 2, 3 — a correct pose up to a symmetry."""
    rng = np.random.default_rng(4)
    q = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    syms = np.stack([np.linalg.matrix_power(q, k) for k in range(4)])
    crops = []
    for k in (1, 2, 3):
        base = rng.normal(size=(40 + 9 * k, 3)) * 6.0
        pts = np.concatenate([R.transform(S, base) for S in syms], 0)
        Tg = gt_pose(rng)
        crops.append(dict(pts=pts, T_gt=Tg, T_est=Tg @ syms[k], syms=syms, k=k))
    return crops, lm_K()
