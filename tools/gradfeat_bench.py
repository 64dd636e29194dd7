"""Device time of each gradient-feature kernel alone at the flagship shape (configs[1]: 64 crops x
1024 points, W = 31 slots, C = 64): 50 launches captured in a HIP graph and replayed (host launch
overhead off the clock), the median of 5 replays. Reports the achieved bytes/s against HBM
(8 TB/s) from the algorithmic bytes — every operand once — and, for the MFMA kernels, flop/s
against the f32 MFMA peak (157.3 TFLOP/s). The operator is a real one: 30 nearest neighbours of
random points on a sphere cap per crop (geometry.build_grad_operator), so the transposed apply
sees a kNN graph's in-degree skew (printed).

  python tools/gradfeat_bench.py [B] [N]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd")]
import torch  # noqa: E402

from dpfm_amd import geometry, ops  # noqa: E402

HBM, MFMA = 8.0e12, 157.3e12
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
LAUNCHES, REPLAYS = 50, 5
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)

# random points on a unit-sphere cap, their normals, the 30-neighbour operator
z = 1.0 - 0.2 * torch.rand(B * N, device=dev, generator=g, dtype=torch.float64)
ph = 6.283185307179586 * torch.rand(B * N, device=dev, generator=g, dtype=torch.float64)
r = (1.0 - z * z).sqrt()
pts = torch.stack((r * ph.cos(), r * ph.sin(), z), dim=1).contiguous()
off = torch.arange(B + 1, device=dev, dtype=torch.int64) * N
nbr, _ = ops.knn(pts, off, N, 30, omit_self=True)
op = geometry.build_grad_operator(pts, off, [N] * B, geometry.tangent_frames(pts), nbr).float()
W = op.idx.shape[2]
deg = (op.tptr[:, 1:] - op.tptr[:, :-1]).float()
print(f"operator B={B} N={N} W={W}: in-degree median {deg.median().item():.0f} max {deg.max().item():.0f}")

R = B * N
cat = torch.randn(B, N, 192, device=dev, generator=g)
dcat = torch.randn(B, N, 192, device=dev, generator=g)
v = torch.empty(B, N, 128, device=dev)
dx = torch.zeros(B, N, 64, device=dev)
A_re = torch.randn(64, 64, device=dev, generator=g) / 8
A_im = torch.randn(64, 64, device=dev, generator=g) / 8
w192 = torch.randn(64, 192, device=dev, generator=g) / 14
b64 = torch.randn(64, device=dev, generator=g)
h1 = torch.empty(R, 64, device=dev)
ops.grad_apply(cat[..., 64:], 192, op.idx, op.val, v)
gbuf = torch.empty(B, N, 64, device=dev)
ops.gradfeat_fwd(v, A_re, A_im, R, gbuf, 64)
dv = torch.randn(B, N, 128, device=dev, generator=g)
opb = 4 * R * W * 3  # the operator: an int32 index and two f32 coefficients per slot

cases = [
    ("grad_apply", lambda: ops.grad_apply(cat[..., 64:], 192, op.idx, op.val, v), 4 * R * (64 + 128) + opb, 0),
    ("grad_apply_t", lambda: ops.grad_apply_t(dv, op.tptr, op.tsrc, op.val, dx, 64, accumulate=True),
     4 * R * (128 + 2 * 64) + opb + 4 * B * (N + 1), 0),
    ("gradfeat_fwd", lambda: ops.gradfeat_fwd(v, A_re, A_im, R, cat[..., 128:], 192), 4 * R * (128 + 64) + 32768,
     2 * R * 128 * 128),
    ("gradfeat_bwd", lambda: ops.gradfeat_bwd(dcat[..., 128:], 192, cat[..., 128:], 192, v, A_re, A_im, R),
     4 * R * (64 + 64 + 128 + 128 + 128) + 32768, 4 * R * 128 * 128),
    ("linear192_fwd", lambda: ops.linear192_fwd(cat, 192, w192, b64, R, True, h1), 4 * R * (192 + 64) + 4 * 64 * 192,
     2 * R * 192 * 64),
]

result = {"B": B, "N": N, "W": W, "indegree_median": deg.median().item(), "indegree_max": deg.max().item(),
          "kernels": {}}
for name, fn, byts, flops in cases:
    for _ in range(3):
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
    us = statistics.median(times)
    bw = byts / us * 1e6
    line = f"{name:14s} {us:7.1f} us (min {min(times):.1f} max {max(times):.1f})  {byts / 1e6:6.1f} MB  " \
           f"{bw / 1e12:5.2f} TB/s = {bw / HBM:.3f} of HBM"
    entry = {"us": us, "bytes": byts, "hbm_share": bw / HBM}
    if flops:
        fl = flops / us * 1e6
        line += f"  {fl / 1e12:6.1f} TFLOP/s = {fl / MFMA:.3f} of the f32 MFMA"
        entry.update(flops=flops, mfma_share=fl / MFMA)
    print(line, flush=True)
    result["kernels"][name] = entry
print(json.dumps(result))
