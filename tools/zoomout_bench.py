"""Device time of ops.zoomout (pk_zoomout: ZoomOut refinement of the 30 x 30 functional map to 64 x 64)
against the same loop written in torch on the same GPU, and what the refinement does on the real crops.

  python tools/zoomout_bench.py                 timing: B = 32 at 1024 x 1024 and at 5000 x 2000, step in {1, 5}
  python tools/zoomout_bench.py --kernels DIR   the split over the kernels: runs itself once per shape under
                                                `rocprofv3 --kernel-trace --stats` (a child process, output in DIR)
  python tools/zoomout_bench.py --real-crops    the seven crops of tests/golden/real_crops.npz through InferStep with
                                                and without zoomout=(64, 5)

Timing: each candidate is captured in a HIP graph (one call per graph), replayed for >= 0.2 s untimed, then
timed over REPLAYS replays between device events; the median is reported with min and max. The torch loop is
the cdist-free expansion |E|^2 - 2 E y^T, argmin, gather and matmul per size. Inputs are seeded random bases
(the time does not depend on the values); the two sides' final point maps are compared before timing (random
bases have no structure to converge to, so the share of equal entries is reported, not asserted).
The nearest-neighbour share of the f32 MFMA peak (155 TFLOP/s) is 2 V1 V2 (4 ceil(k / 4)) B flop per size over
the zo_nn_kernel time of the kernel trace.
"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dpfm_amd import ops  # noqa: E402

F32_MFMA = 155e12
SHAPES = ((32, 1024, 1024), (32, 5000, 2000))
STEPS = (1, 5)
REPLAYS, WARM_S = 7, 0.2
if not torch.cuda.is_available():
    raise SystemExit("zoomout_bench needs a HIP device (no CPU timing path)")
dev = torch.device("cuda:0")


def inputs(B, V1, V2, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ex = torch.randn(B, V1, 64, generator=g, device=dev)
    ey = torch.randn(B, V2, 64, generator=g, device=dev)
    mass = torch.full((B, V2), 1.0 / V2, device=dev)
    C0 = torch.eye(30, device=dev)[None] + 0.15 * torch.randn(B, 30, 30, generator=g, device=dev)
    n1 = torch.full((B,), V1, dtype=torch.int32, device=dev)
    n2 = torch.full((B,), V2, dtype=torch.int32, device=dev)
    return ex, ey, mass, C0.contiguous(), n1, n2


def torch_zoomout(ex, ey, mass, C0, k_final, step):
    C = C0
    ks = ops.zoomout_schedule(k_final, step)
    for it, k in enumerate(ks):
        E = ex[..., :k] @ C.transpose(1, 2)
        s = (E * E).sum(-1)[..., None] - 2.0 * (E @ ey[..., :k].transpose(1, 2))
        p = s.argmin(1)
        if it + 1 < len(ks):
            kn = ks[it + 1]
            C = (ey[..., :kn] * mass[..., None]).transpose(1, 2) @ torch.gather(
                ex[..., :kn], 1, p[..., None].expand(-1, -1, kn))
    return C, p


def nn_flops(B, V1, V2, k_final, step):
    return sum(2.0 * B * V1 * V2 * 4 * ((k + 3) // 4) for k in ops.zoomout_schedule(k_final, step))


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
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
        times.append(e0.elapsed_time(e1))
    del gr
    return dict(ms=statistics.median(times), min=min(times), max=max(times))


def timing():
    result = {"replays": REPLAYS, "cases": []}
    for B, V1, V2 in SHAPES:
        ex, ey, mass, C0, n1, n2 = inputs(B, V1, V2)
        nbytes = int(ops._lib.lib().pk_zoomout_work_size(B, V1, V2, 64, 1))
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for step in STEPS:
            C, p = ops.zoomout(ex, ey, mass, C0, n1, n2, 64, step, work=work)
            Ct, pt = torch_zoomout(ex, ey, mass, C0, 64, step)
            same = float((p == pt).float().mean())
            hip = timed(lambda: ops.zoomout(ex, ey, mass, C0, n1, n2, 64, step, work=work))
            base = timed(lambda: torch_zoomout(ex, ey, mass, C0, 64, step))
            fl = nn_flops(B, V1, V2, 64, step)
            case = dict(B=B, V1=V1, V2=V2, step=step, sizes=len(ops.zoomout_schedule(64, step)), hip=hip, torch=base,
                        ratio_torch_over_hip=base["ms"] / hip["ms"], nn_flops=fl,
                        whole_call_share_of_f32_mfma_peak=fl / (hip["ms"] * 1e-3) / F32_MFMA,
                        final_map_equal_share=same, work_bytes=nbytes)
            result["cases"].append(case)
            print(f"B {B} {V1} x {V2} step {step}: hip {hip['ms']:8.3f} ms [{hip['min']:.3f}, {hip['max']:.3f}]  torch "
                  f"{base['ms']:8.3f} ms [{base['min']:.3f}, {base['max']:.3f}]  torch/hip {case['ratio_torch_over_hip']:.2f}"
                  f"  NN flop over the whole call {case['whole_call_share_of_f32_mfma_peak']:.3f} of 155 TF  "
                  f"final maps equal on {same:.4f}", flush=True)
        del ex, ey, work
        torch.cuda.empty_cache()
    print(json.dumps(result))


PIECES = (("nearest neighbour", ("zo_nn_kernel",)), ("nn merge", ("zo_nn_merge",)), ("embed", ("zo_embed", "zo_ylayout")),
          ("project", ("zo_project", "zo_reduce", "zo_copy")))


def kernels_child(B, V1, V2, step, calls):
    ex, ey, mass, C0, n1, n2 = inputs(B, V1, V2)
    for _ in range(calls):
        ops.zoomout(ex, ey, mass, C0, n1, n2, 64, step)
    torch.cuda.synchronize()


def kernels(outdir):
    """One traced child per (shape, step): CALLS calls of ops.zoomout, the kernel stats summed per piece."""
    calls = 3
    result = {"calls_per_trace": calls, "cases": []}
    for B, V1, V2 in SHAPES:
        for step in STEPS:
            d = os.path.join(outdir, f"zoomout_trace_B{B}_{V1}x{V2}_s{step}")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "zo", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--kernels-child", str(B), str(V1), str(V2), str(step),
                   str(calls)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            case = dict(B=B, V1=V1, V2=V2, step=step)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not files:
                case["error"] = f"rocprofv3 rc {r.returncode}, {len(files)} stats files: not measured"
                print(case["error"], r.stderr[-400:], flush=True)
                result["cases"].append(case)
                continue
            ns = {name: 0.0 for name, _ in PIECES}
            other = 0.0
            for row in csv.DictReader(open(files[0])):
                tot = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
                kn = row.get("Name") or row.get("KernelName") or ""
                for name, keys in PIECES:
                    if any(k in kn for k in keys) and not (name == "nearest neighbour" and "merge" in kn):
                        ns[name] += tot
                        break
                else:
                    other += tot
            per_call_ms = {k: v / calls * 1e-6 for k, v in ns.items()}
            fl = nn_flops(B, V1, V2, 64, step)
            nn_ms = per_call_ms["nearest neighbour"]
            case.update(per_call_ms=per_call_ms, other_kernels_ms=other / calls * 1e-6,
                        nn_share_of_f32_mfma_peak=(fl / (nn_ms * 1e-3) / F32_MFMA) if nn_ms > 0 else None)
            result["cases"].append(case)
            print(f"B {B} {V1} x {V2} step {step}: " + "  ".join(f"{k} {v:.3f} ms" for k, v in per_call_ms.items()) +
                  f"  (other kernels of the process {case['other_kernels_ms']:.3f} ms)  NN at "
                  f"{case['nn_share_of_f32_mfma_peak']} of 155 TF", flush=True)
    print(json.dumps(result))


def real_crops():
    """InferStep on the seven real crops with the crops' and CADs' own point-cloud operators (64
    eigenvectors, geometry.point_cloud_operators) and seeded random-initialised weights (the repository
    ships no trained weights), with and without zoomout=(64, 5)."""
    from dpfm_amd import geometry
    from dpfm_amd.dataset.object import Crops, FrameBatch
    from dpfm_amd.models.dpfm import DPFMNet
    from dpfm_amd.pipeline import InferStep, Operators, pad_rows
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_crops.npz"))
    cs = []
    for k in range(int(g["n"])):
        T = g[f"{k}_T_gt"]
        cs.append(dict(pc=g[f"{k}_pc"], R=T[:3, :3].copy(), t=T[:3, 3].copy(), cad=g[f"cad_{int(g[f'{k}_obj_id'])}"],
                       diam=float(g[f"{k}_diam"])))
    n1 = [len(c["cad"]) for c in cs]
    n2 = [len(c["pc"]) for c in cs]
    ld = max(n2)

    def spectral(arrs, counts, pad):
        off = ops.packed_offsets(counts, dev)
        pts = torch.from_numpy(np.concatenate(arrs)).to(dev).float().double()
        so = geometry.point_cloud_operators(pts, off, counts, k_eig=64)
        ev = torch.zeros(len(counts), pad, 64, device=dev)
        ms = torch.zeros(len(counts), pad, device=dev)
        ev[:, :so.evecs.shape[1]] = so.evecs.float()
        ms[:, :so.mass.shape[1]] = so.mass.float()
        return ms, so.evals.float().contiguous(), ev

    t0 = time.perf_counter()
    cm, ce, cv = spectral([c["cad"] for c in cs], n1, max(n1))
    pm, pe, pv = spectral([c["pc"] for c in cs], n2, ld)
    torch.cuda.synchronize()
    t_ops = time.perf_counter() - t0
    diam = [c["diam"] for c in cs]
    T_ = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    op = Operators(cad_mass=cm, cad_evals=ce, cad_evecs=cv,
                   cad_xyz=T_(pad_rows([np.asarray(c["cad"], np.float64).astype(np.float32) for c in cs])),
                   pc_mass=pm, pc_evals=pe, pc_evecs=pv,
                   ir_thr=torch.tensor([np.float32(0.1 * x) for x in diam], dtype=torch.float32, device=dev),
                   rig_thr=ops.rigidity_thresholds(diam, dev), cad_n=torch.tensor(n1, dtype=torch.int32, device=dev))
    pc_off = ops.packed_offsets(n2, dev)
    pc64 = torch.from_numpy(np.concatenate([c["pc"] for c in cs])).to(dev)
    pc32, n2t = ops.collate_pad(pc64, pc_off, ld)
    al = torch.from_numpy(np.concatenate([(c["pc"] - c["t"]) @ c["R"] for c in cs])).to(dev)  # R^T (p - t) per row
    al32, _ = ops.collate_pad(al, pc_off, ld)
    fb = FrameBatch(depth=None, mask=None, rgb=None, K=None, cam_scale=None,
                    R=torch.from_numpy(np.stack([c["R"].reshape(9) for c in cs])).to(dev),
                    t=torch.from_numpy(np.stack([c["t"] for c in cs])).to(dev),
                    cad64=torch.from_numpy(np.concatenate([c["cad"] for c in cs])).to(dev),
                    cad_off=ops.packed_offsets(n1, dev), diam=diam, max_pixels=0, thr2=None, n1max=max(n1))
    crops = Crops(pc64=pc64, pc32=pc32, align64=al, align32=al32, off=pc_off, n2=n2t, ld=ld, npoint=None, pairs=None,
                  npairs=None, overlap_12=None, overlap_21=None, rgb=None, kept=None)
    torch.manual_seed(1)
    model = DPFMNet().to(dev).eval()
    out = {"operators_seconds": round(t_ops, 2), "n1": n1, "n2": n2, "weights": "random init, torch.manual_seed(1)"}
    for name, zo in (("top5", None), ("zoomout_64_5", (64, 5))):
        r = InferStep(model, hypotheses=1024, seed=3, zoomout=zo)(fb, op, crops)
        torch.cuda.synchronize()
        out[name] = dict(survivors=r["n_corr"].cpu().tolist(), ir=[round(float(x), 4) for x in r["ir"].cpu()],
                         metrics=[[round(float(v), 4) for v in row] for row in r["metrics"].cpu()])
        print(name, json.dumps(out[name]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels-child":
        kernels_child(*(int(a) for a in sys.argv[2:7]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles"))
    elif len(sys.argv) > 1 and sys.argv[1] == "--real-crops":
        real_crops()
    else:
        timing()
