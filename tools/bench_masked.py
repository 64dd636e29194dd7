"""Masked mode against the unmasked path at the same padded shape, in the same build.

B = 32 crops padded to 2000 points, true lengths drawn uniformly from [115, 2000] (fixed seed):
  attn_fwd      ops.attention forward                      (work ratio: sum n m / (B N M))
  attn_fwd_bwd  ops.attention forward + backward           (same)
  instnorm      ops.instnorm_relu forward + backward, C=64 (work ratio: sum n / (B N))
  train_step    one eager TrainStep.forward_backward at the reference's sizes (ragged crops of
                the sample policy padded to 2000, CADs of ~2000 vertices); its lengths are the
                crop formation's own, and its work ratio is reported for the attention part
Per step: warm-up, then REPS timed repetitions of masked and unmasked alternating (device events
around INNER calls each); median, min and max per variant, the time ratio of the medians and the
work ratio the lengths leave. A kernel cannot beat its work ratio; how far above it the time
ratio sits is what the tool is for.

  python tools/bench_masked.py            # every step, each a child process under its own
                                          # `timeout`; stops at the first failure; writes
                                          # profiles/masked_bench.json
  python tools/bench_masked.py --step attn_fwd   # one step in this process, JSON on stdout
The run fails when masked attention (forward, or forward + backward) is slower than unmasked.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd")
for _p in (ROOT, PKG_ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEPS = {"attn_fwd": 120, "attn_fwd_bwd": 120, "instnorm": 120, "train_step": 420}  # name -> time limit (s)
B, N, LO, HI, SEED = 32, 2000, 115, 2000, 0
D, H, C = 16, 2, 64


def lengths():
    import numpy as np
    rng = np.random.default_rng(SEED)
    return rng.integers(LO, HI + 1, size=B).tolist(), rng.integers(LO, HI + 1, size=B).tolist()


def stats(ms):
    s = sorted(ms)
    n = len(s)
    med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    return {"median_ms": round(med, 5), "min_ms": round(s[0], 5), "max_ms": round(s[-1], 5), "reps": n}


def alternate(variants: dict, warmup: int, reps: int, inner: int) -> dict:
    """name -> thunk. Every variant is warmed up, then the variants are timed in turn, `reps`
    times, each repetition `inner` calls between two device events."""
    import torch
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return {k: stats(v) for k, v in times.items()}


def report(step: str, res: dict, work_ratio: float, extra=None) -> dict:
    ratio = res["masked"]["median_ms"] / res["unmasked"]["median_ms"]
    out = {"step": step, "masked": res["masked"], "unmasked": res["unmasked"], "time_ratio": round(ratio, 4),
           "work_ratio": round(work_ratio, 4)}
    out.update(extra or {})
    return out


def step_attention(backward: bool, args) -> dict:
    import torch
    from dpfm_amd import ops
    dev = torch.device("cuda:0")
    qlen, klen = lengths()
    g = torch.Generator().manual_seed(SEED)
    q, k, v, go = (torch.randn(B, D, H, N, generator=g).to(dev) for _ in range(4))
    ql = torch.tensor(qlen, dtype=torch.int32, device=dev)
    kl = torch.tensor(klen, dtype=torch.int32, device=dev)
    if backward:
        q, k, v = (t.requires_grad_() for t in (q, k, v))

    def run(masked):
        def fn():
            out = ops.attention(q, k, v, ql, kl) if masked else ops.attention(q, k, v)
            if backward:
                q.grad = k.grad = v.grad = None
                out.backward(go)
        return fn

    ctx = torch.enable_grad() if backward else torch.no_grad()
    with ctx:
        res = alternate({"unmasked": run(False), "masked": run(True)}, args.warmup, args.reps, args.inner)
    work = sum(a * b for a, b in zip(qlen, klen)) / (B * N * N)
    return report("attn_fwd_bwd" if backward else "attn_fwd", res, work,
                  {"shape": f"B={B} D={D} H={H} N=M={N}", "len_min": min(qlen + klen), "len_max": max(qlen + klen)})


def step_instnorm(args) -> dict:
    import torch
    from dpfm_amd import ops
    dev = torch.device("cuda:0")
    qlen, _ = lengths()
    g = torch.Generator().manual_seed(SEED)
    x = (torch.randn(B, C, N, generator=g) * 3 + 1).to(dev).requires_grad_()
    dy = torch.randn(B, C, N, generator=g).to(dev)
    ln = torch.tensor(qlen, dtype=torch.int32, device=dev)

    def run(masked):
        def fn():
            x.grad = None
            (ops.instnorm_relu(x, 1e-5, ln) if masked else ops.instnorm_relu(x, 1e-5)).backward(dy)
        return fn

    res = alternate({"unmasked": run(False), "masked": run(True)}, args.warmup, args.reps, args.inner)
    return report("instnorm", res, sum(qlen) / (B * N), {"shape": f"B={B} C={C} N={N}"})


def step_train(args) -> dict:
    import torch
    from dpfm_amd.dataset.object import CropFormation
    from dpfm_amd.dataset.synthetic import ragged_frames
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import TrainStep, frame_batch, operators_for
    dev = torch.device("cuda:0")
    frames = ragged_frames(B, 77, n1=N)
    fb = frame_batch(frames, dev)
    crops = CropFormation(npoint=0, seed=0, pad="fixed")(fb)
    counts = crops.n2.cpu().tolist()
    op = operators_for([f["cad"] for f in frames], counts, fb.diam, 0, dev, ld2=crops.ld)
    cads = [len(f["cad"]) for f in frames]
    torch.manual_seed(1234)
    plain, masked = DPFMNet().to(dev), DPFMNet(masked=True).to(dev)
    masked.load_state_dict(plain.state_dict())
    steps = {"unmasked": TrainStep(plain, seed=1), "masked": TrainStep(masked, seed=1, masked=True)}
    res = alternate({k: (lambda s=s: s.forward_backward(op, crops)) for k, s in steps.items()},
                    max(2, args.warmup // 2), args.reps, 1)
    n1max, ld = op.cad_xyz.shape[1], crops.ld
    work = sum(a * b for a, b in zip(cads, counts)) / (B * n1max * ld)
    return report("train_step", res, work,
                  {"shape": f"B={B} eager forward_backward, crops {min(counts)}-{max(counts)} padded to {ld}, "
                            f"CADs {min(cads)}-{max(cads)} padded to {n1max}",
                   "note": "work_ratio is the attention's (sum n1 n2 / (B N1 N2)); the encoder, the heads and "
                           "the loss are per point and run at the padded size in both variants"})


def run_step(name: str, args) -> dict:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_masked.py measures on a HIP device: none found (no CPU fallback)")
    if name == "attn_fwd":
        return step_attention(False, args)
    if name == "attn_fwd_bwd":
        return step_attention(True, args)
    if name == "instnorm":
        return step_instnorm(args)
    return step_train(args)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions per variant (>= 20)")
    ap.add_argument("--inner", type=int, default=5, help="calls per repetition (kernel steps)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_bench.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("bench_masked.py: --reps must be at least 20")
    if args.step:
        print(json.dumps(run_step(args.step, args)))
        return 0
    results = []
    for name, limit in STEPS.items():  # each GPU step a fresh process under its own time limit
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
               "--warmup", str(args.warmup), "--reps", str(args.reps), "--inner", str(args.inner)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"bench_masked.py: step {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode or 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        results.append(r)
        print(f"{name:13s} masked {r['masked']['median_ms']:9.4f} ms [{r['masked']['min_ms']:.4f}, "
              f"{r['masked']['max_ms']:.4f}]  unmasked {r['unmasked']['median_ms']:9.4f} ms "
              f"[{r['unmasked']['min_ms']:.4f}, {r['unmasked']['max_ms']:.4f}]  time ratio {r['time_ratio']:.3f}  "
              f"work ratio {r['work_ratio']:.3f}", flush=True)
    doc = {"lengths": f"uniform [{LO}, {HI}], seed {SEED}, B={B}, padded to {N}", "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    slow = [r["step"] for r in results if r["step"].startswith("attn") and r["time_ratio"] > 1.0]
    if slow:
        print(f"bench_masked.py: masked attention slower than unmasked: {slow}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
