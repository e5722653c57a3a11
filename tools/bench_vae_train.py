"""Time one AutoencoderKL optimizer step on the engine (``VAETrainStep.step``) for the model block of the reference's
``configs/LDCT/LDCT_autoencoder_kl.json`` (82.6 M parameters, 256x256, batch 4, synthetic input, the config's own
training block: l1, kl_weight 1e-6, no GAN, no perceptual term), with ``VAEEngine.kl_forward`` on the same model as
the yardstick.

    python tools/bench_vae_train.py [--out profiles/vae_train_bench.jsonl] [--batch 4] [--steps 10] [--repeats 5]

Protocol: 3 warm-up calls of each arm, then ``--repeats`` windows per arm, alternating, each ``--steps`` calls
between two HIP events after a device synchronise.  One JSON line: the median, minimum and maximum ms per call of
each arm over the windows, the step-to-forward ratio of the medians, the kernel launches of one step and of one
forward (torch.profiler; null if it is not available), and the step's share of the dense bf16 MFMA peak at 3 x the
forward FLOPs (269.2 + 618.7 GFLOP per image for encode + decode).  There is no earlier VAE
train step to compare with: the numbers are recorded, not gated.  Needs a ROCm GPU; it never falls back."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flow-matching-and-diffusion-models_amd"))

LDCT_VAE = dict(in_channels=1, out_channels=1, resolution=256, base_ch=128, down_channels=[128, 256, 512, 512],
                num_res_blocks=2, attn_resolutions=[], z_channels=4, embed_dim=4, dropout=0.0, use_attention=True,
                spatial_dims=2, emb_channels=None, use_scale_shift_norm=False, double_z=True, attn_heads=4,
                attn_dim_head=64)
LDCT_TRAINING = {"learning_rate": 1e-4, "weight_decay": 0.0, "kl_weight": 1e-6, "kl_anneal_steps": 0, "reg_type": "kl",
                 "recon_type": "l1", "perceptual_weight": 0.0, "gan_weight": 0.0}
FWD_GFLOP_PER_IMAGE = 269.2 + 618.7
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA


def _launches(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and not e.name.lower().startswith(("memcpy", "memset")))
    except Exception:   # noqa: BLE001 - the count is optional, the timings are not
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_vae_train needs a ROCm GPU"
    from fmdiff.models.vae import AutoencoderKL
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime.vae_engine import get_vae_engine
    torch.cuda.set_stream(torch.cuda.Stream())
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = AutoencoderKL(**LDCT_VAE).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    img = torch.rand(a.batch, 1, 256, 256, device="cuda", generator=g)
    eps = torch.randn(a.batch, 4, 32, 32, device="cuda", generator=g)
    step = VAETrainStep(vae, LDCT_TRAINING)
    eng = get_vae_engine(vae)
    xin = vae.image_to_model_range(img)
    arms = {"step": lambda: step.step(img, eps), "forward": lambda: eng.kl_forward(xin, eps)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(a.repeats):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                out = fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.steps)
    loss = float(step.step(img, eps)["loss"])
    launches = {k: _launches(fn) for k, fn in arms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    tflops = 3 * FWD_GFLOP_PER_IMAGE * a.batch / med["step"]   # GFLOP / ms = TFLOP/s
    rec = dict(workload=f"AutoencoderKL (LDCT_autoencoder_kl) train step, 256x256, batch {a.batch}, eager",
               params=sum(p.numel() for p in vae.parameters()), steps_per_window=a.steps, windows=a.repeats,
               step_ms=dict(median=med["step"], min=min(ms["step"]), max=max(ms["step"])),
               forward_ms=dict(median=med["forward"], min=min(ms["forward"]), max=max(ms["forward"])),
               step_to_forward=med["step"] / med["forward"], launches=launches, step_tflops=tflops,
               step_mfma_frac=tflops / PEAK_BF16_TFLOPS, loss_after=loss, global_step=step.global_step)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
