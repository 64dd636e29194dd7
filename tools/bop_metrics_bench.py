"""Device time of ops.bop_errors (pk_bop_errors: MSSD, MSPD, ADI) at the reference's evaluation
shape — B = 32 crops, V = 5,000 CAD vertices, S in {1, 8, 630} symmetries per crop — against a
device fp64 torch expression of the same quantities on the same machine:

  ADI          torch.cdist(T_est x, T_gt y).min(-1).values.mean(-1)
  MSSD / MSPD  einsum over (symmetry, vertex), norm, amax over vertices, amin over symmetries

Each candidate is captured in a HIP graph (LAUNCHES calls per graph, host launch overhead off the
clock), replayed for >= 60 ms untimed, then timed over REPLAYS replays between device events; the
median is reported with min and max. The ADI share of the fp64 VALU peak (78.6 TFLOP/s) counts 9 flop
per (query, target) pair — 3 subtractions, 1 multiply, 2 FMAs, 1 min — over the time of the
`adi_only` call (S = 1, no K): that call also runs the prep, symmetry and finish launches, so the
share is a lower bound of the ADI kernel's own. Outputs of the two sides are compared before timing.

  python tools/bop_metrics_bench.py [B] [V]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd")]
import torch  # noqa: E402

from dpfm_amd import ops  # noqa: E402

F64_VALU = 78.6e12
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
V = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
SYMS = (1, 8, 630)
LAUNCHES, REPLAYS, WARM_S = 4, 7, 0.06
if not torch.cuda.is_available():
    raise SystemExit("bop_metrics_bench needs a HIP device (no CPU timing path)")
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
f64 = dict(dtype=torch.float64, device=dev)


def rot(axis, ang):
    a = axis / axis.norm(dim=-1, keepdim=True)
    Kx = torch.zeros(*a.shape[:-1], 3, 3, **f64)
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -a[..., 2], a[..., 1], a[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -a[..., 0], -a[..., 1], a[..., 0]
    c, s = torch.cos(ang)[..., None, None], torch.sin(ang)[..., None, None]
    return c * torch.eye(3, **f64) + s * Kx + (1 - c) * a[..., :, None] * a[..., None, :]


def rigid(R, t):
    T = torch.zeros(*R.shape[:-2], 4, 4, **f64)
    T[..., :3, :3], T[..., :3, 3], T[..., 3, 3] = R, t, 1.0
    return T


pts = torch.randn(B, V, 3, generator=g, **f64) * 6.0
cad = pts.reshape(-1, 3).contiguous()
off = torch.arange(B + 1, device=dev, dtype=torch.int64) * V
T_gt = rigid(rot(torch.randn(B, 3, generator=g, **f64), torch.rand(B, generator=g, **f64) * 3),
             torch.randn(B, 3, generator=g, **f64) * 3 + torch.tensor([2.0, -3.0, 80.0], **f64))
T_est = T_gt @ rigid(rot(torch.randn(B, 3, generator=g, **f64), torch.full((B,), 0.05, **f64)),
                     torch.randn(B, 3, generator=g, **f64) * 1.0)
K = torch.tensor([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], **f64).expand(B, 3, 3)
K = K.contiguous()


def sym_set(S):  # S rotations about z through an offset, the same set for every crop
    ang = torch.arange(S, **f64) * (2 * torch.pi / S)
    R = rot(torch.tensor([0.0, 0.0, 1.0], **f64).expand(S, 3), ang)
    o = torch.tensor([0.3, -0.2, 0.0], **f64)
    return rigid(R, o - R @ o).repeat(B, 1, 1).contiguous(), torch.arange(B + 1, device=dev, dtype=torch.int64) * S


def tf(T, x):  # [B,4,4] x [B,V,3]
    return x @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]


def torch_adi():
    return torch.cdist(tf(T_est, pts), tf(T_gt, pts)).min(-1).values.mean(-1)


def torch_sym(sym):  # -> (MSSD, MSPD)
    S = sym.shape[0] // B
    M = T_gt[:, None] @ sym.view(B, S, 4, 4)
    gp = torch.einsum("bsij,bvj->bsvi", M[..., :3, :3], pts) + M[:, :, None, :3, 3]
    ep = tf(T_est, pts)
    d3 = (ep[:, None] - gp).norm(dim=-1).amax(-1).amin(-1)
    pg = torch.einsum("bij,bsvj->bsvi", K, gp)
    pe = torch.einsum("bij,bvj->bvi", K, ep)
    d2 = ((pe[..., :2] / pe[..., 2:])[:, None] - pg[..., :2] / pg[..., 2:]).norm(dim=-1).amax(-1).amin(-1)
    return d3, d2


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            for _ in range(LAUNCHES):
                fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        gr.replay()
        torch.cuda.synchronize()
    times = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    del gr
    return dict(us=statistics.median(times), min=min(times), max=max(times))


result = {"B": B, "V": V, "launches_per_graph": LAUNCHES, "replays": REPLAYS, "cases": {}}

# ADI alone (S = 1, no K) against cdist
out, _ = ops.bop_errors(cad, off, V, T_est, T_gt)
ref = torch_adi()
result["adi_max_abs_diff_vs_torch"] = float((out[:, 2] - ref).abs().max())
hip = timed(lambda: ops.bop_errors(cad, off, V, T_est, T_gt))
base = timed(torch_adi)
flops = 9.0 * B * V * V
share = flops / (hip["us"] * 1e-6) / F64_VALU
result["cases"]["adi_only"] = dict(hip=hip, torch=base, ratio_torch_over_hip=base["us"] / hip["us"], flops=flops,
                                   fp64_valu_share_lower_bound=share)
print(f"adi_only     hip {hip['us']:9.1f} us [{hip['min']:.1f}, {hip['max']:.1f}]  torch {base['us']:9.1f} us "
      f"[{base['min']:.1f}, {base['max']:.1f}]  torch/hip {base['us'] / hip['us']:.2f}  "
      f"ADI >= {share:.3f} of the fp64 VALU peak", flush=True)

for S in SYMS:
    sym, sym_off = sym_set(S)
    out, best = ops.bop_errors(cad, off, V, T_est, T_gt, K, sym, sym_off, S)
    d3, d2 = torch_sym(sym)
    diff = max(float((out[:, 0] - d3).abs().max()), float((out[:, 1] - d2).abs().max()),
               float((out[:, 2] - ref).abs().max()))
    hip = timed(lambda: ops.bop_errors(cad, off, V, T_est, T_gt, K, sym, sym_off, S))
    base = timed(lambda: (torch_adi(), torch_sym(sym)))
    result["cases"][f"S{S}"] = dict(hip=hip, torch=base, ratio_torch_over_hip=base["us"] / hip["us"],
                                    max_abs_diff_vs_torch=diff)
    print(f"all three S={S:<3d} hip {hip['us']:9.1f} us [{hip['min']:.1f}, {hip['max']:.1f}]  torch {base['us']:9.1f} us "
          f"[{base['min']:.1f}, {base['max']:.1f}]  torch/hip {base['us'] / hip['us']:.2f}  max |diff| {diff:.2e}",
          flush=True)
print(json.dumps(result))
