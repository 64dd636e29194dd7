"""numpy fp64 restatement of the BOP pose errors (bop_toolkit pose_error.py mssd / mspd / adi) and
of the symmetry-set construction (misc.get_symmetry_transformations), written naively: a Python loop
over the symmetries, the full V x V distance matrix for ADI. Independent of dpfm_amd (formats.py and
the kernels are checked against this file, not the other way round).

bop_toolkit itself is not a dependency of the tests, so these are the project's definitions:
  MSSD = min_S max_x ||T_est x - T_gt S x||
  MSPD = min_S max_x ||proj(K, T_est x) - proj(K, T_gt S x)||, proj(K, p) = (K p)[:2] / (K p)[2]
  ADI  = mean_x min_y ||T_est x - T_gt y||
with the first minimum reported as the best symmetry."""
import math

import numpy as np


def transform(T, pts):
    return pts @ T[:3, :3].T + T[:3, 3]


def project(K, p):
    q = p @ K.T
    return q[:, :2] / q[:, 2:3]


def mssd_all(T_est, T_gt, pts, syms):
    """The per-symmetry maxima (the list MSSD is the minimum of)."""
    e = transform(T_est, pts)
    out = []
    for S in syms:
        g = transform(T_gt, transform(S, pts))
        out.append(np.linalg.norm(e - g, axis=1).max())
    return np.array(out)


def mspd_all(T_est, T_gt, K, pts, syms):
    e = project(K, transform(T_est, pts))
    out = []
    for S in syms:
        g = project(K, transform(T_gt, transform(S, pts)))
        out.append(np.linalg.norm(e - g, axis=1).max())
    return np.array(out)


def adi(T_est, T_gt, pts):
    e = transform(T_est, pts)
    g = transform(T_gt, pts)
    d = np.linalg.norm(e[:, None, :] - g[None, :, :], axis=2)
    return d.min(axis=1).mean()


def add(T_est, T_gt, pts):
    return np.linalg.norm(transform(T_est, pts) - transform(T_gt, pts), axis=1).mean()


def errors(T_est, T_gt, K, pts, syms):
    """dict(mssd, mspd, adi, best=(i3, i2), all3, all2, scale3, scale2): the three errors, the
    first-argmin symmetries, the per-symmetry lists and the magnitudes the tolerance is stated in
    (largest absolute transformed coordinate; largest absolute pixel coordinate)."""
    a3 = mssd_all(T_est, T_gt, pts, syms)
    a2 = mspd_all(T_est, T_gt, K, pts, syms)
    e, g = transform(T_est, pts), transform(T_gt, pts)
    scale3 = max(np.abs(e).max(), np.abs(g).max())
    scale2 = max(np.abs(project(K, e)).max(), np.abs(project(K, g)).max())
    return dict(mssd=a3.min(), mspd=a2.min(), adi=adi(T_est, T_gt, pts), best=(int(a3.argmin()), int(a2.argmin())),
                all3=a3, all2=a2, scale3=scale3, scale2=scale2)


def rotation(angle, axis):
    """Rotation matrix by `angle` about `axis`, column by column from the axis-angle formula
    v' = v cos + (a x v) sin + a (a . v)(1 - cos)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / math.sqrt(float(a @ a))
    R = np.zeros((3, 3))
    for j in range(3):
        v = np.zeros(3)
        v[j] = 1.0
        R[:, j] = v * math.cos(angle) + np.cross(a, v) * math.sin(angle) + a * float(a @ v) * (1.0 - math.cos(angle))
    return R


def symmetry_transformations(info, max_sym_disc_step=0.01, scale=0.1):
    """[S, 4, 4]: identity + discrete, each combined with every discretised continuous rotation
    (C D, discrete outer, continuous inner, i = 0 included); translations * scale."""
    disc = [np.eye(4)]
    for v in info.get("symmetries_discrete", []):
        disc.append(np.array(v, dtype=np.float64).reshape(4, 4))
    cont = []
    for c in info.get("symmetries_continuous", []):
        n = int(math.ceil(math.pi / max_sym_disc_step))
        off = np.array(c["offset"], dtype=np.float64)
        for i in range(n):
            T = np.eye(4)
            T[:3, :3] = rotation(2.0 * math.pi * i / n, c["axis"])
            T[:3, 3] = off - T[:3, :3] @ off
            cont.append(T)
    out = []
    for D in disc:
        if cont:
            for C in cont:
                out.append(C @ D)
        else:
            out.append(D.copy())
    out = np.stack(out)
    out[:, :3, 3] = out[:, :3, 3] * scale
    return out
