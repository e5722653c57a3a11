"""Time one EMA training step of the vector quantizer (quantize + EMA update + backward) on the HIP kernels
(``VectorQuantizerEMA.quantize_train_nhwc``: csrc/vq.hip + csrc/vq_train.hip) against the reference's formula in
fp32 torch on the same GPU (src/nn/modules/vae/codebook.py:109-137: distances, argmin, one-hot, two matmuls, the
in-place EMA, autograd).

    python tools/bench_vq_train.py [--out profiles/vq_train_bench.jsonl] [--seconds 0.5] [--pairs 3]

The protocol of tools/bench_vq.py: per shape (M, K, D) seeded inputs of two kinds, ``clustered`` (z = e_j + 0.05 n
around the initial codebook with j uniform: every code keeps a few rows, a healthy tokenizer) and ``randn``
(unrelated to the codebook: the EMA pulls the used codes towards the data mean and within the window a few codes
take most rows, a collapsing codebook and the update kernel's worst case, one long segment; the record carries
the longest segment of a step after the window).  The timed steps rotate through latent
buffers that together hold ``--rotate-mb`` (320 MB, more than the Infinity Cache); HIP events around a window of
about ``--seconds`` (the step count comes from a 20-step estimate, never under 50) after 3 warm-up steps; the two
arms alternate over ``--pairs`` pairs.  Every arm of every pair runs in a process of its own under
``--arm-timeout`` seconds, one at a time; the first arm that fails or runs out of time ends the run.  One JSON
line per (shape, pair, arm): microseconds per step, peak bytes torch allocated during the steps, and for the HIP
arm its workspace bytes (argmin workspace, codebook planes, the saved z - q, the fp64 n).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flow-matching-and-diffusion-models_amd"))

SHAPES = ((4096, 16384, 256), (8192, 16384, 256), (8192, 512, 64))
BETA, DECAY, EPS = 0.25, 0.99, 1e-5


def arm(a):
    import torch
    import torch.nn.functional as F

    from fmdiff import _lib
    from fmdiff.nn.modules.vae import VectorQuantizerEMA
    from fmdiff.runtime import ops
    assert torch.cuda.is_available(), "bench_vq_train needs a ROCm GPU"
    M, K, D = SHAPES[a.shape]
    a.inputs = a.inputs or "clustered"
    g = torch.Generator(device="cuda").manual_seed(M + K + D)
    m = VectorQuantizerEMA(K, D, BETA, decay=DECAY, eps=EPS).to("cuda").train()
    with torch.no_grad():
        m.embedding.copy_(torch.randn(K, D, generator=g, device="cuda"))
        m.ema_w.copy_(m.embedding)
        m.ema_cluster_size.fill_(1.0)
    ninputs = int(a.rotate_mb * 1e6 / (4 * M * D)) + 1
    zs = [torch.randn(1, M, D, generator=g, device="cuda") for _ in range(ninputs)]
    if a.inputs == "clustered":
        zs = [m.embedding[torch.randint(0, K, (M,), generator=g, device="cuda")][None] + 0.05 * z for z in zs]
    zs = [z.requires_grad_() for z in zs]
    g_zq = torch.randn(1, D, M, generator=g, device="cuda")
    g_loss = torch.tensor(0.7, device="cuda")

    def hip(z):
        out = m.quantize_train_nhwc(z)
        torch.autograd.backward([out.zq, out.vq_loss], [g_zq, g_loss])
        z.grad = None
        return out

    def torch_fp32(z):
        flat = z[0]
        e = m.embedding
        d = (flat ** 2).sum(1, keepdim=True) + (e ** 2).sum(1) - 2.0 * torch.matmul(flat, e.t())
        idx = torch.argmin(d, dim=1)
        enc = F.one_hot(idx, K).type(flat.dtype)
        q = torch.matmul(enc, e)
        with torch.no_grad():
            m.ema_cluster_size.mul_(DECAY).add_(enc.sum(0), alpha=1 - DECAY)
            m.ema_w.mul_(DECAY).add_(torch.matmul(enc.t(), flat.detach()), alpha=1 - DECAY)
            n = m.ema_cluster_size.sum()
            cl = (m.ema_cluster_size + EPS) / (n + K * EPS) * n
            m.embedding.copy_(m.ema_w / cl.unsqueeze(1))
        zq = (flat + (q - flat).detach()).t()[None]
        loss = BETA * F.mse_loss(q.detach(), flat)
        torch.autograd.backward([zq, loss], [g_zq, g_loss])
        z.grad = None

    fn = hip if a.arm == "hip" else torch_fp32

    def window(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(n):
            fn(zs[i % len(zs)])
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e-3

    for i in range(3):
        fn(zs[i % len(zs)])
    torch.cuda.synchronize()
    iters = max(50, int(a.seconds / (window(20) / 20)) + 1)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    total = window(iters)
    rec = dict(M=M, K=K, D=D, inputs=a.inputs, pair=a.pair, arm=a.arm, us=round(total * 1e6 / iters, 2), steps=iters,
               window_s=round(total, 3), rotating_inputs=ninputs,
               peak_alloc_bytes=int(torch.cuda.max_memory_allocated() - base),
               finite=bool(torch.isfinite(m.embedding).all()))
    if a.arm == "hip":
        planes = sum(t.numel() * t.element_size() for t in ops.vq_codebook_planes(m.embedding))
        cpw, grid = ops.vq_train_plan(M, K, D)
        rec.update(workspace_bytes=int(_lib.lib().fmd_vq_workspace(M, K, D)) + planes + 4 * M * D + 8,
                   workspace_bytes_per_row=round((int(_lib.lib().fmd_vq_workspace(M, K, D)) + 4 * M * D + 8) / M, 1),
                   codebook_plane_bytes=planes, segsum_codes_per_wg=cpw, segsum_grid=grid,
                   longest_segment=int(hip(zs[0]).hist.max()))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rotate-mb", type=float, default=320.0)
    ap.add_argument("--arm-timeout", type=float, default=90.0)
    ap.add_argument("--inputs", choices=("clustered", "randn"), default=None)
    ap.add_argument("--arm", choices=("hip", "torch_fp32"), default=None)
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--pair", type=int, default=0)
    a = ap.parse_args()
    if a.arm:
        return arm(a)
    lines = []
    for shape, inputs in ((s, i) for s in range(len(SHAPES)) for i in ((a.inputs,) if a.inputs else ("clustered", "randn"))):
        for pair in range(a.pairs):
            for which in ("hip", "torch_fp32"):
                cmd = [sys.executable, os.path.abspath(__file__), "--arm", which, "--shape", str(shape), "--pair",
                       str(pair), "--seconds", str(a.seconds), "--rotate-mb", str(a.rotate_mb), "--inputs", inputs]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.arm_timeout)
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"{which} at {SHAPES[shape]} ran past {a.arm_timeout} s: stopping")
                if r.returncode != 0:
                    raise SystemExit(f"{which} at {SHAPES[shape]} failed ({r.returncode}): stopping\n{r.stderr[-2000:]}")
                lines.append(r.stdout.strip().splitlines()[-1])
                print(lines[-1], flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
