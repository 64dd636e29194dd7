"""Quick per-kernel timing (development aid): FPS and ball query at C2/C4 sizes."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "6d-pose-estimation-for-unseen-categories_amd")]
import numpy as np
import torch
from dpfm_amd import ops

dev = torch.device("cuda:0")

def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters

rng = np.random.default_rng(0)
from dpfm_amd import _lib  # noqa: E402
_lib.use_dev_lib()  # pkdev_* hooks: libposekern_dev.so (Makefile)
from dpfm_amd.pipeline import make_frame_batch  # noqa: E402

L = _lib.lib()
# FPS on real crop-formation output (pixel-ordered SOR survivors of synthetic frames)
for B, npt in [(32, 1024)]:
    fb, _ = make_frame_batch(B, 1024, 1024, seed=0, device=dev)
    bp = ops.backproject(fb.depth, fb.mask, fb.K, fb.cam_scale, cap=B * fb.max_pixels)
    so = ops.sor(bp["xyz"], bp["off"], fb.max_pixels, 20, 0.3, pix=bp["pix"], idxmap=bp["idxmap"], K=fb.K)
    ms = timeit(lambda: ops.backproject(fb.depth, fb.mask, fb.K, fb.cam_scale, cap=B * fb.max_pixels), iters=5, warm=1)
    print(f"backproject B={B}: {ms:.3f} ms")
    ms = timeit(lambda: ops.sor(bp["xyz"], bp["off"], fb.max_pixels, 20, 0.3, pix=bp["pix"], idxmap=bp["idxmap"], K=fb.K),
                iters=5, warm=1)
    ms0 = timeit(lambda: ops.sor(bp["xyz"], bp["off"], fb.max_pixels, 20, 0.3, pix=bp["pix"], idxmap=bp["idxmap"]),
                 iters=3, warm=1)
    print(f"sor B={B} n={(bp['off'][1:] - bp['off'][:-1]).tolist()[:4]}...: {ms:.3f} ms with K box, {ms0:.3f} ms 5x5 only")
    x, off = so["xyz32"], so["off"]
    nin = int((off[1:] - off[:-1]).max())
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    npv = torch.full((B,), npt, dtype=torch.int32, device=dev)
    ref = ops.fps_packed(x, off, nin, st, npv, npt)
    ms = timeit(lambda: ops.fps_packed(x, off, nin, st, npv, npt), iters=5, warm=1)
    print(f"fps (dispatch) B={B} n_in<={nin} npoint={npt}: {ms:.3f} ms  ({ms*1e3/npt:.3f} us/iter)")
    out = torch.zeros((B, npt), dtype=torch.int64, device=dev)
    for mode in (4, 3):  # the flat and the per-lane kernel, whatever the dispatch would pick
        f = lambda: L.pkdev_fps_cfg(_lib.ptr(x), _lib.ptr(off), B, nin, _lib.ptr(st), _lib.ptr(npv), _lib.ptr(out),
                                    npt, 1024, mode, _lib.stream(dev))
        if f() != 0:
            continue
        ms = timeit(f, iters=20, warm=5)
        print(f"   mode={mode}: {ms:.3f} ms ({ms*1e3/npt:.3f} us/iter) same={torch.equal(out, ref)}")

if len(sys.argv) > 1 and sys.argv[1] == "fps":
    sys.exit(0)
for B, N in [(32, 1024), (256, 2048)]:
    cad = torch.from_numpy(rng.normal(size=(B * N, 3)) * 5).to(dev)
    pc = torch.from_numpy(rng.normal(size=(B * N, 3)) * 5).to(dev)
    off = ops.packed_offsets([N] * B, dev)
    thr = torch.full((B,), ops.ball_threshold(0.6), dtype=torch.float64, device=dev)
    ld = N
    mask = torch.empty((B, N, ld), dtype=torch.uint8, device=dev)
    rc = torch.empty((B, N), dtype=torch.int32, device=dev)
    from dpfm_amd._lib import call, ptr, stream
    s = stream(dev)
    f = lambda: call("pk_ball_query_mask", ptr(cad), ptr(off), ptr(pc), ptr(off), ptr(thr), B, N, N, ptr(mask), ld, ptr(rc), s)
    ms = timeit(f)
    byts = B * (24 * N + 24 * N + N * N)
    print(f"ball_query_mask (f32 screen) B={B} N={N}: {ms:.3f} ms, {byts/ms/1e6:.1f} GB/s algorithmic")
    # dense case: a large share of the pairs within r, many near the boundary
    thr_d = torch.full((B,), ops.ball_threshold(8.0), dtype=torch.float64, device=dev)
    fd = lambda: call("pk_ball_query_mask", ptr(cad), ptr(off), ptr(pc), ptr(off), ptr(thr_d), B, N, N, ptr(mask), ld, ptr(rc), s)
    ms = timeit(fd)
    print(f"ball_query_mask dense (r=8, {float(rc.double().mean())/N:.3f} in) B={B} N={N}: {ms:.3f} ms, "
          f"{byts/ms/1e6:.1f} GB/s")
    f2 = lambda: ops.ball_query(cad, off, pc, off, [0.6] * B, N, N, 64 * N, thr2=thr)
    ms = timeit(f2)
    print(f"ball_query full (mask+scan+pairs) B={B} N={N}: {ms:.3f} ms")
    f3 = lambda: ops.ball_query(cad, off, pc, off, [0.6] * B, N, N, 64 * N, with_mask=False, thr2=thr)
    ms = timeit(f3)
    print(f"ball_query fused (count+scan+pairs, no mask) B={B} N={N}: {ms:.3f} ms")

# per-point layer weight gradients
for (R_or_B, I, O, N, cf) in [(65536, 128, 64, 0, False), (65536, 64, 64, 0, False), (65536, 64, 32, 0, False),
                              (32, 64, 64, 1024, True), (32, 32, 32, 1024, True)]:
    if cf:
        x = torch.randn(R_or_B, I, N, device=dev)
        dy = torch.randn(R_or_B, O, N, device=dev)
        R = R_or_B * N
    else:
        x = torch.randn(R_or_B, I, device=dev)
        dy = torch.randn(R_or_B, O, device=dev)
        R = R_or_B
    ms2 = timeit(lambda: ops.linear_wgrad(x, dy, channels_first=cf))
    fl = 2.0 * R * I * O
    print(f"linear_wgrad R={R} I={I} O={O} {'cf' if cf else 'cl'}: {ms2*1e3:.1f} us ({fl/ms2/1e9:.1f} TF/s)")

# per-point layer forward / input gradient: pk_linear_fwd vs the library GEMM (+ bias)
for (R_or_B, I, O, N, cf) in [(65536, 128, 64, 0, False), (65536, 64, 128, 0, False), (65536, 3, 64, 0, False),
                              (32, 64, 64, 1024, True), (32, 32, 64, 1024, True), (32, 128, 32, 1024, True)]:
    x = torch.randn(R_or_B, I, N, device=dev) if cf else torch.randn(R_or_B, I, device=dev)
    w = torch.randn(O, I, device=dev)
    b = torch.randn(O, device=dev)
    R = R_or_B * (N if cf else 1)
    y = ops.linear_fwd(x, w, b, channels_first=cf)
    if cf:
        ref = lambda: torch.bmm(w.expand(R_or_B, -1, -1), x).add_(b[:, None])
    else:
        ref = lambda: torch.addmm(b, x, w.t())
    rel = float((y - ref()).abs().max() / ref().abs().max())
    ms = timeit(lambda: ops.linear_fwd(x, w, b, channels_first=cf))
    msr = timeit(ref)
    bts = 4.0 * R * (I + O)
    print(f"linear_fwd R={R} I={I} O={O} {'cf' if cf else 'cl'}: {ms*1e3:.1f} us ({bts/ms/1e6:.0f} GB/s) "
          f"torch {msr*1e3:.1f} us; max rel diff {rel:.2e}", flush=True)
