"""CPU census of sor_knn_kernel's control flow (csrc/crop.hip) on the bench's own frames: what a
64-lane wave executes against what its lanes need. No GPU.

  python tools/sor_wave_census.py [first_seed last_seed]     (default 0 1; the bench uses 0..7)

Per wave (64 consecutive row-major points of a crop) it replays the 5x5 / 9x9 / 17x17 window
choice, T, the camera box and the guarded insertions of the box scan, and reports
  - the share of waves that run each window retry and the lanes that need it,
  - insertion steps executed by the wave (a step runs when any lane inserts at that loop
    position) against the insertions a lane needs,
  - box-scan gather steps of the wave (the union of its lanes' loop positions) against the lane mean,
and from those the compare-exchange count per wave of the round-6 kernel (every retry rebuilds
the list: 25 + 81 (+ 289) full insertions) and of the present one (25 pixels as a fixed sequence
of 290 exchanges, rings added with guarded insertions)."""
import bisect
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd")]
from oracle import dpfm_oracle as O  # noqa: E402
from dpfm_amd.dataset.synthetic import make_frame  # noqa: E402

KNN, BATCH, MAXBOX = 20, 4, 1024


def box_of(K, H, W, u, v, q, T):
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    r = math.sqrt(T) * (1.0 + 1e-9) + 1e-300
    if not (q[2] > r):
        return None
    rho = r / q[2]
    tx = min(max(abs(cx), abs(W - 1 - cx)) / fx, (abs(q[0] / q[2]) + rho) / (1.0 - rho))
    ty = min(max(abs(cy), abs(H - 1 - cy)) / fy, (abs(q[1] / q[2]) + rho) / (1.0 - rho))
    bu, bv = fx * rho * math.sqrt(1 + tx * tx), fy * rho * math.sqrt(1 + ty * ty)
    if not (bu < 64 and bv < 64):
        return None
    ru, rv = math.ceil(bu * (1 + 1e-9)) + 1, math.ceil(bv * (1 + 1e-9)) + 1
    if (2 * ru + 1) * (2 * rv + 1) > MAXBOX:
        return None
    return max(u - ru, 0), min(u + ru, W - 1), max(v - rv, 0), min(v + rv, H - 1)


def scan(idx, xyz, q, u, v, Rw, rect, T, best, guard_T):
    """The kernel's rectangle-minus-window loop: -> (gather positions, insertion positions)."""
    u0, u1, v0, v1 = rect
    gathers, inserts = [], []
    for vv in range(v0, v1 + 1):
        in_w = v - Rw <= vv <= v + Rw
        segs = [(u0, min(u1, u - Rw - 1)), (max(u0, u + Rw + 1), u1)] if in_w else [(u0, u1)]
        for sg, (a, c) in enumerate(segs):
            for k, uu in enumerate(range(a, c + 1, BATCH)):
                gathers.append((vv - v0, sg, k))
                for t in range(min(BATCH, c - uu + 1)):
                    j = idx[vv, uu + t]
                    if j < 0:
                        continue
                    d = xyz[j] - q
                    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    if (not guard_T or s <= T) and (len(best) < KNN or s < best[KNN - 1]):
                        bisect.insort(best, s)
                        del best[KNN:]
                        inserts.append((vv - v0, sg, k, t))
    return gathers, inserts


def main():
    lo, hi = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (0, 1)
    tot = dict(waves=0, w9=0, w17=0, l9=0, l17=0, ring_wave=0, ring_lane=0, box_ins_wave=0, box_ins_lane=0,
               box_step_wave=0, box_step_lane=0, lanes=0, brute=0)
    for seed in range(lo, hi + 1):
        f = make_frame(seed)
        E = O.erode_seg_mask(f.mask == 255)
        xyz = O.dpt_2_pcld(f.depth, 1000 / f.depth_scale, f.K, f.mask == 255)
        H, W = E.shape
        idx = -np.ones((H, W), dtype=np.int64)
        idx[E] = np.arange(xyz.shape[0])
        vs, us = np.nonzero(E)
        n = xyz.shape[0]
        kk = min(KNN, n)
        for w0 in range(0, n, 64):
            g_union, i_union, r_union = set(), set(), set()
            lanes = range(w0, min(w0 + 64, n))
            need9 = need17 = 0
            for i in lanes:
                u, v, q = int(us[i]), int(vs[i]), xyz[i]
                win = idx[max(v - 2, 0):v + 3, max(u - 2, 0):u + 3]
                pts = win[win >= 0]
                d = xyz[pts] - q
                best = sorted(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).tolist())[:KNN]
                found, Rw = pts.size, 2
                while found < kk and Rw > 0:
                    R = 2 * Rw
                    if R > 8:
                        Rw = -1
                        break
                    rect = (max(u - R, 0), min(u + R, W - 1), max(v - R, 0), min(v + R, H - 1))
                    g, ins = scan(idx, xyz, q, u, v, Rw, rect, math.inf, best, False)
                    found = int((idx[rect[2]:rect[3] + 1, rect[0]:rect[1] + 1] >= 0).sum())
                    r_union |= {(R,) + k for k in ins}
                    tot["ring_lane"] += len(ins)
                    need9 += R == 4
                    need17 += R == 8
                    Rw = R
                box = box_of(f.K, H, W, u, v, q, best[kk - 1]) if Rw > 0 else None
                if box is None:
                    tot["brute"] += 1
                    continue
                g, ins = scan(idx, xyz, q, u, v, Rw, box, best[kk - 1], best, True)
                g_union |= set(g)
                i_union |= set(ins)
                tot["box_ins_lane"] += len(ins)
                tot["box_step_lane"] += len(g)
            tot["waves"] += 1
            tot["lanes"] += len(lanes)
            tot["w9"] += need9 > 0
            tot["w17"] += need17 > 0
            tot["l9"] += need9
            tot["l17"] += need17
            tot["ring_wave"] += len(r_union)
            tot["box_ins_wave"] += len(i_union)
            tot["box_step_wave"] += len(g_union)
    wv, ln = tot["waves"], tot["lanes"]
    print(f"seeds {lo}..{hi}: {wv} waves, {ln} queries, {tot['brute']} to the brute force")
    print(f"waves running the 9x9 retry {100 * tot['w9'] / wv:.1f} % for {tot['l9'] / max(tot['w9'], 1):.1f} lanes; "
          f"17x17 {100 * tot['w17'] / wv:.1f} % for {tot['l17'] / max(tot['w17'], 1):.1f} lanes")
    print(f"box scan per wave: {tot['box_ins_wave'] / wv:.1f} insertion steps executed, {tot['box_ins_lane'] / ln:.2f} "
          f"insertions needed per lane; {tot['box_step_wave'] / wv:.1f} gather steps executed, lane mean "
          f"{tot['box_step_lane'] / ln:.1f}")
    print(f"ring scans per wave: {tot['ring_wave'] / wv:.1f} guarded insertion steps executed "
          f"({tot['ring_lane'] / max(tot['l9'] + tot['l17'], 1):.1f} per lane that retries)")
    old = 20 * (25 + 81 * tot["w9"] / wv + 289 * tot["w17"] / wv + tot["box_ins_wave"] / wv)
    new = 290 + 20 * (tot["ring_wave"] / wv + tot["box_ins_wave"] / wv)
    print(f"compare-exchanges per wave: round-6 kernel {old:.0f} (3 fp64 VALU each with the canonicalising max: "
          f"{3 * old:.0f}), present kernel {new:.0f} (2 each: {2 * new:.0f})")


if __name__ == "__main__":
    main()
