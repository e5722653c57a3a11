"""Time ops.image_metrics (csrc/metrics.hip) against the path it replaces: a device-to-host copy of both batches and
the reference's CPU arithmetic (per image the clamp, the squared error and skimage's structural_similarity
defaults on float32, restated here with scipy.ndimage.uniform_filter because skimage is not a dependency), run
over the images of the batch on at most 16 CPU threads.

    python tools/bench_metrics.py [--out profiles/metrics_bench.jsonl] [--seconds 0.5] [--pairs 3]

Per shape: seeded inputs in [-0.1, 1.1]; the HIP calls rotate through input pairs that together hold
``--rotate-mb`` (320 MB, more than the 256 MB Infinity Cache, so an input is not cache-resident when its turn comes
again); HIP events around a window of about ``--seconds`` (the call count comes from a 20-call estimate, never
under 200) after 3 warm-up calls; nothing synchronises inside the window.  The CPU path is timed with the wall
clock over ``--cpu-reps`` calls, each including its device-to-host copy.  The two alternate over ``--pairs``
pairs.  One JSON line per (shape, pair, implementation): microseconds per call; for the HIP path also the bytes of
both inputs over the time (GB/s of compulsory traffic), the workspace bytes and the worst |ssim - ssim_cpu32|
against the CPU path's float32 value (informative: the fp64 value is the one returned on purpose).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flow-matching-and-diffusion-models_amd"))

from fmdiff import _lib  # noqa: E402
from fmdiff.runtime import ops  # noqa: E402

SHAPES = ((8, 1, 256, 256), (1, 1, 128, 128, 128))
CPU_THREADS = 16


def _ssim32(x, y):
    """skimage.metrics.structural_similarity(x, y, channel_axis=None, data_range=1.0) on float32 arrays."""
    from scipy.ndimage import uniform_filter
    npix = 7.0 ** x.ndim
    cov = npix / (npix - 1.0)
    ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
    vx = cov * (uniform_filter(x * x, size=7) - ux * ux)
    vy = cov * (uniform_filter(y * y, size=7) - uy * uy)
    vxy = cov * (uniform_filter(x * y, size=7) - ux * uy)
    s = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux ** 2 + uy ** 2 + 1e-4) * (vx + vy + 9e-4))
    return float(s[tuple(slice(3, n - 3) for n in s.shape)].mean(dtype=np.float64))


def _cpu_image(g, t):
    g, t = np.clip(g, 0.0, 1.0), np.clip(t, 0.0, 1.0)
    mse = float(np.mean((g - t) ** 2))
    return mse, 10.0 * np.log10(1.0 / max(mse, 1e-12)), float(np.mean([_ssim32(g[c], t[c]) for c in range(g.shape[0])]))


def cpu_path(gen, tgt, pool):
    """Device tensors in, the three per-image lists out: the copy and the reference's arithmetic."""
    g, t = gen.cpu().numpy(), tgt.cpu().numpy()
    return list(pool.map(_cpu_image, g, t))


def _window(fn, pairs, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(n):
        fn(*pairs[i % len(pairs)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3


def timed_hip(fn, pairs, seconds):
    for i in range(3):
        fn(*pairs[i % len(pairs)])
    torch.cuda.synchronize()
    iters = max(200, int(seconds / (_window(fn, pairs, 20) / 20)) + 1)
    total = _window(fn, pairs, iters)
    return total * 1e6 / iters, iters, total


def timed_cpu(pairs, pool, reps):
    cpu_path(*pairs[0], pool)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        cpu_path(*pairs[i % len(pairs)], pool)
    total = time.perf_counter() - t0
    return total * 1e6 / reps, reps, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--rotate-mb", type=float, default=320.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics needs a ROCm GPU"
    lines = []
    for shape in SHAPES:
        N, C, sp = shape[0], shape[1], shape[2:]
        g = torch.Generator(device="cuda").manual_seed(sum(shape))
        nbytes = 2 * 4 * int(np.prod(shape))
        npairs = int(a.rotate_mb * 1e6 / nbytes) + 1
        pairs = []
        for _ in range(npairs):
            tgt = 1.2 * torch.rand(shape, generator=g, device="cuda") - 0.1
            pairs.append((tgt + 0.05 * torch.randn(shape, generator=g, device="cuda"), tgt))
        ws = int(_lib.lib().fmd_image_metrics_workspace(N, C, *((0,) * (3 - len(sp)) + tuple(sp))))
        hip = lambda x, y: ops.image_metrics(x, y, clamp=True)
        threads = min(CPU_THREADS, N)
        with cf.ThreadPoolExecutor(max_workers=threads) as pool:
            want = cpu_path(*pairs[0], pool)
            got = hip(*pairs[0]).stacked.cpu().numpy()
            diff = max(abs(got[2][i] - want[i][2]) for i in range(N))
            for pair in range(a.pairs):
                us, iters, total = timed_hip(hip, pairs, a.seconds)
                rec = dict(shape=list(shape), pair=pair, impl="hip", us=round(us, 2), calls=iters,
                           window_s=round(total, 3), rotating_inputs=npairs, input_gb_per_s=round(nbytes / us * 1e-3, 1),
                           workspace_bytes=ws, ssim_vs_cpu_float32=float(f"{diff:.3e}"))
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                us, iters, total = timed_cpu(pairs, pool, a.cpu_reps)
                rec = dict(shape=list(shape), pair=pair, impl="copy_and_scipy_float32", us=round(us, 1), calls=iters,
                           window_s=round(total, 3), cpu_threads=threads)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
