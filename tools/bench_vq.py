"""Time the HIP vector quantizer (ops.vq_quantize, csrc/vq.hip) against the reference's formula in fp32 torch
(``z_sq + e_sq - 2 z @ e.T`` -> argmin -> gather, src/nn/modules/vae/codebook.py:70-76) on the same GPU.

    python tools/bench_vq.py [--out profiles/vq_bench.jsonl] [--seconds 0.5] [--pairs 3]

Per shape (M, K, D): seeded randn inputs; the timed calls rotate through latent buffers that together hold
``--rotate-mb`` (320 MB, more than the 256 MB Infinity Cache, so a latent is not cache-resident when its turn
comes again; the codebook is a model parameter and stays where repeated calls leave it); HIP events around a
window of about ``--seconds`` (the call count comes from a 20-call estimate, never under 200) after 3
warm-up calls; the two implementations alternate over ``--pairs`` pairs.  One
JSON line per (shape, pair, implementation): microseconds per call, and for the HIP path the fraction of the
bf16 dense peak counting the three MFMA products (3 x 2 M K D flop), its workspace bytes (argmin workspace, and
the cached codebook planes) and the peak bytes torch allocated during the calls for both.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flow-matching-and-diffusion-models_amd"))

from fmdiff import _lib  # noqa: E402
from fmdiff.runtime import ops  # noqa: E402

BF16_PEAK = 2.5e15   # MI355X dense bf16 flop/s
SHAPES = ((4096, 16384, 256), (8192, 16384, 256), (8192, 512, 64))


def torch_formula(z, e):
    d = (z ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2.0 * torch.matmul(z, e.t())
    idx = torch.argmin(d, dim=1)
    return idx, e[idx]


def _window(fn, zs, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(n):
        fn(zs[i % len(zs)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3


def timed(fn, zs, seconds):
    for i in range(3):
        fn(zs[i % len(zs)])
    torch.cuda.synchronize()
    iters = max(200, int(seconds / (_window(fn, zs, 20) / 20)) + 1)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    total = _window(fn, zs, iters)
    return total * 1e6 / iters, torch.cuda.max_memory_allocated() - base, iters, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rotate-mb", type=float, default=320.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vq needs a ROCm GPU"
    lines = []
    for M, K, D in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + K + D)
        e = torch.randn(K, D, generator=g, device="cuda")
        ninputs = int(a.rotate_mb * 1e6 / (4 * M * D)) + 1
        zs = [torch.randn(M, D, generator=g, device="cuda") for _ in range(ninputs)]
        plan = ops.vq_plan(M, K, D)
        ws = int(_lib.lib().fmd_vq_workspace(M, K, D))
        planes = sum(t.numel() * t.element_size() for t in ops.vq_codebook_planes(e))
        hip = lambda z: ops.vq_quantize(z, D, e, 0.25, False)
        agree = float((hip(zs[0]).codes == torch_formula(zs[0], e)[0]).double().mean())
        for pair in range(a.pairs):
            for impl, fn in (("hip", hip), ("torch_fp32", lambda z: torch_formula(z, e))):
                us, peak, iters, total = timed(fn, zs, a.seconds)
                rec = dict(M=M, K=K, D=D, pair=pair, impl=impl, us=round(us, 2), calls=iters,
                           window_s=round(total, 3), rotating_inputs=ninputs, peak_alloc_bytes=int(peak))
                if impl == "hip":
                    rec.update(splits=plan.splits, bf16_peak_fraction=round(3 * 2.0 * M * K * D / (us * 1e-6) / BF16_PEAK, 4),
                               workspace_bytes=ws, codebook_plane_bytes=planes, codes_equal_torch=round(agree, 5))
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
