"""Time one whole VAE criterion step (forward + backward, KL configuration) on the HIP criterion kernels
(fmdiff.nn.losses / reparameterize_kl / VAECriterion, csrc/vae_loss.hip) against the same formulas in eager fp32
torch with autograd on the same GPU.

    python tools/bench_vae_loss.py [--out profiles/vae_loss_bench.jsonl] [--seconds 0.5] [--pairs 3]

A step is: posterior sample + KL from the moments, the reconstruction loss of the raw decoder output, ``total =
recon + kl_scale * kl.mean()``, and the backward to the decoder output and the moments (z receives a fixed
upstream gradient, as the decoder's backward would supply).  Shapes: 8x1x256x256 with moments 8x8x32x32, and the
3-D 2x1x32x128x128 with moments 2x8x4x16x16; recon_type l1 and bce_focal.

Protocol of tools/bench_vq.py: seeded inputs rotating through ``--rotate-mb`` (320 MB, more than the 256 MB Infinity
Cache); HIP events around a window of about ``--seconds`` (call count from a 20-call estimate, never under 200)
after 3 warm-up calls; the two arms alternate over ``--pairs`` pairs.  Each (shape, recon_type, pair, arm) runs in
its own process (``--child``) under its own time limit, so an arm cannot disturb the other's allocator or
clocks.  One JSON line each: microseconds per step and the kernel launches of one step (counted with
torch.profiler; null if the profiler is not available).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flow-matching-and-diffusion-models_amd"))

SHAPES = (((8, 1, 256, 256), (8, 8, 32, 32)), ((2, 1, 32, 128, 128), (2, 8, 4, 16, 16)))
RECON = ("l1", "bce_focal")
CFG = {"kl_weight": 1e-4, "kl_anneal_steps": 1000}
STEP = 100


def torch_step(recon_type, kl_scale):
    import torch
    import torch.nn.functional as F

    def step(rec, target, moments, eps, g_z):
        mu, logvar = torch.chunk(moments, 2, dim=1)
        logvar = torch.clamp(logvar, -30.0, 20.0)
        z = mu + torch.exp(0.5 * logvar) * eps
        kl = 0.5 * torch.sum(mu.pow(2) + torch.exp(logvar) - 1.0 - logvar, dim=tuple(range(1, mu.ndim)))
        if recon_type == "l1":
            recon = F.l1_loss((rec.clamp(-1.0, 1.0) + 1.0) * 0.5, target)
        else:
            prob = torch.sigmoid(rec)
            ce = F.binary_cross_entropy_with_logits(rec, target, reduction="none")
            p_t = prob * target + (1 - prob) * (1 - target)
            alpha_t = 0.25 * target + 0.75 * (1 - target)
            recon = F.binary_cross_entropy_with_logits(rec, target) + (alpha_t * (1 - p_t).pow(2.0) * ce).mean()
        total = recon + kl_scale * kl.mean()
        torch.autograd.backward([total, z], [None, g_z])
        return total
    return step


def hip_step(recon_type):
    from fmdiff.nn.modules.vae import reparameterize_kl
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    import torch
    crit = VAECriterion(dict(CFG, recon_type=recon_type))

    def step(rec, target, moments, eps, g_z):
        z, kl = reparameterize_kl(moments, eps)
        out = crit(rec, target, kl=kl, global_step=STEP)
        torch.autograd.backward([out["loss"], z], [None, g_z])
        return out["loss"]
    return step, crit.kl_scale(STEP)


def child(a):
    import torch
    assert torch.cuda.is_available(), "bench_vae_loss needs a ROCm GPU"
    shape, mshape = SHAPES[a.shape]
    g = torch.Generator(device="cuda").manual_seed(17 + a.shape)
    per_set = 4 * (2 * torch.Size(shape).numel() + 3 * torch.Size(mshape).numel())
    nsets = int(a.rotate_mb * 1e6 / per_set) + 1
    eshape = (mshape[0], mshape[1] // 2, *mshape[2:])
    sets = []
    for _ in range(nsets):
        sets.append((torch.randn(shape, generator=g, device="cuda").requires_grad_(),
                     torch.rand(shape, generator=g, device="cuda"),
                     torch.randn(mshape, generator=g, device="cuda").requires_grad_(),
                     torch.randn(eshape, generator=g, device="cuda"), torch.randn(eshape, generator=g, device="cuda")))
    hip, kl_scale = hip_step(a.recon)
    fn = hip if a.arm == "hip" else torch_step(a.recon, kl_scale)

    def call(i):
        s = sets[i % nsets]
        s[0].grad = None
        s[2].grad = None
        return fn(*s)

    def window(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(n):
            call(i)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e-3

    for i in range(3):
        call(i)
    torch.cuda.synchronize()
    iters = max(200, int(a.seconds / (window(20) / 20)) + 1)
    total = window(iters)
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call(0)
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower())
    except Exception as e:   # the profiler is optional
        print(f"profiler unavailable: {e}", file=sys.stderr)
    loss = float(call(0))
    print(json.dumps(dict(shape=list(shape), moments=list(mshape), recon_type=a.recon, pair=a.pair, arm=a.arm,
                          us=round(total * 1e6 / iters, 2), calls=iters, window_s=round(total, 3),
                          rotating_sets=nsets, launches=launches, loss=loss)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rotate-mb", type=float, default=320.0)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of one arm's process, seconds")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--arm", default="hip")
    ap.add_argument("--shape", type=int, default=0)
    ap.add_argument("--recon", default="l1")
    ap.add_argument("--pair", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []
    for si in range(len(SHAPES)):
        for recon in RECON:
            for pair in range(a.pairs):
                for arm in ("hip", "torch_fp32"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--shape", str(si),
                           "--recon", recon, "--pair", str(pair), "--seconds", str(a.seconds), "--rotate-mb",
                           str(a.rotate_mb)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                    if r.returncode != 0:   # nothing more is started on the GPU after a failed arm
                        sys.stderr.write(r.stderr)
                        raise SystemExit(f"{arm} arm failed with status {r.returncode}")
                    lines.append(r.stdout.strip().splitlines()[-1])
                    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
