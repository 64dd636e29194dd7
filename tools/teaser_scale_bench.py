"""TEASER++ scale estimation on the device, measured alone: python tools/teaser_scale_bench.py

Fixed shapes B = 32 x n = 2000 and B = 1 x n = 2000 correspondences (40 % planted inliers, scale
1.7, seeded). After two warm-up calls per shape, the medians of 7 replays of pk_teaser_scale and
pk_teaser_graph_scaled (HIP events around each call), then — in a separate pass, the tracer slows
the host — the per-kernel times of 5 replays from torch.profiler's device activity (`--no-trace`
skips it, e.g. under an external kernel tracer). The sort's achieved bytes/s is its algorithmic
traffic (per radix pass: the histogram reads the 8 B keys, the scatter reads and writes the 12 B
records: 32 B per endpoint) over the summed time of its four kernels, as a fraction of the 8 TB/s
HBM peak. The CPU baseline is the numpy restatement (tests/_teaser_scale_ref.py) on one crop of
the same input, times B. One JSON line per shape."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _teaser_scale_ref as R  # noqa: E402
from dpfm_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12
BETA = 0.1
SORT = ("scale_hist_kernel", "scale_scan_tiles_kernel", "scale_scan_digits_kernel", "scale_scatter_kernel")


def timed(fn, replays):
    out = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def kernel_times(fn, replays):
    """name -> device ms per replay (summed over the kernel's launches in one call)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(replays):
            fn()
        torch.cuda.synchronize()
    acc = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            acc[ev.name] = acc.get(ev.name, 0.0) + ev.device_time / 1e3  # us -> ms
    short = {}
    for name, ms in acc.items():
        key = next((k for k in SORT + ("scale_emit_kernel", "scale_partial_kernel", "scale_carry_kernel",
                                       "scale_apply_kernel", "scale_final_kernel", "teaser_graph_scaled_kernel")
                    if k in name), None)
        if key:
            short[key] = short.get(key, 0.0) + ms / replays
    return short


def main():
    trace = "--no-trace" not in sys.argv
    dev = torch.device("cuda:0")
    for B, n in ((32, 2000), (1, 2000)):
        rng = np.random.default_rng(100 + B)
        crops = [R.planted_scaled(rng, n, 0.4, 1.7)[:2] for _ in range(B)]
        a = torch.from_numpy(np.concatenate([c[0] for c in crops])).to(dev)
        b = torch.from_numpy(np.concatenate([c[1] for c in crops])).to(dev)
        off = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
        nbytes = int(_lib.lib().pk_teaser_scale_work_size(B, n))
        work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        state = {}

        def vote():
            state["scale"], state["info"] = ops.teaser_scale(a, b, off, n, BETA, work=work)

        def graph():
            state["adj"] = ops.teaser_graph(a, b, off, n, BETA, scale=state["scale"])

        for _ in range(2):
            vote()
            graph()
        torch.cuda.synchronize()
        t_vote, t_graph = timed(vote, 7), timed(graph, 7)
        endpoints = B * n * (n - 1)
        res = {"B": B, "n": n, "endpoints": endpoints, "work_bytes": nbytes,
               "teaser_scale_ms": statistics.median(t_vote), "teaser_scale_ms_min_max": [min(t_vote), max(t_vote)],
               "teaser_graph_scaled_ms": statistics.median(t_graph),
               "scale": [float(x) for x in state["scale"][:2].cpu()]}
        if trace:
            k = kernel_times(lambda: (vote(), graph()), 5)
            res["kernel_ms"] = {name: round(ms, 4) for name, ms in sorted(k.items())}
            sort_ms = sum(k.get(name, 0.0) for name in SORT)
            if sort_ms > 0:
                res["sort_ms"] = sort_ms
                res["sort_bytes_per_s"] = 8 * 32 * endpoints / (sort_ms * 1e-3)
                res["sort_fraction_of_hbm_peak"] = res["sort_bytes_per_s"] / HBM_PEAK
        t0 = time.perf_counter()
        v = R.scale_vote(crops[0][0], crops[0][1], BETA)
        R.scaled_graph(crops[0][0], crops[0][1], BETA, v["scale"])
        res["numpy_reference_ms"] = (time.perf_counter() - t0) * 1e3 * B  # one crop measured, times B
        res["numpy_scale"] = v["scale"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
