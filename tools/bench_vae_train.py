"""Time one AutoencoderKL optimizer step on the engine (``VAETrainStep.step``) for the model block of the reference's
``configs/LDCT/LDCT_autoencoder_kl.json`` (82.6 M parameters, 256x256, batch 4, synthetic input, the config's own
training block: l1, kl_weight 1e-6, no GAN, no perceptual term), with ``VAEEngine.kl_forward`` on the same model as
the yardstick; the same for the VQVAE of ``configs/LDCT/LDCT_vqvae.json`` (EMA codebook) and
``LDCT_vqvae_original.json`` (classic codebook) with ``VAEEngine.vq_forward`` as the yardstick (``--arm vq_ema`` /
``vq_classic``); and an A/B of the latent-join kernel against the four-pass composition it replaces at
M = 4 x 32 x 32 rows, D = 256 (``--arm join``; eager calls at this size measure the host's launch rate, ``--graph``
replays a captured graph of 50 calls of each arm and measures the device).  ``--perceptual`` (or ``--arm perc``)
times ``VGGPerceptualLoss`` forward + backward alone (full-width VGG16 stack, random weights, batch 8,
1 x 256 x 256 -> 224 x 224), the AutoencoderKL step with and without the term (perceptual_weight 1.0), and records the
kernel ``fmd_conv_plan`` chooses for each of the ten convs at 224 x 224 and batch 8.

    python tools/bench_vae_train.py [--arm kl|vq_ema|vq_classic|join|gan|perc|all] [--perceptual] [--out profiles/vae_train_bench.jsonl]
                                    [--batch 4] [--steps 10] [--repeats 5]

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
LDCT_VQ = dict(in_channels=1, out_channels=1, resolution=256, base_ch=32, down_channels=[32, 64, 128, 256],
               num_res_blocks=2, attn_resolutions=[], z_channels=256, embed_dim=256, dropout=0.0, use_attention=False,
               spatial_dims=2, emb_channels=None, use_scale_shift_norm=False, attn_heads=1, attn_dim_head=64,
               codebook_size=16384, vq_beta=0.25, vq_ema_decay=0.99, vq_ema_eps=1e-5)
LDCT_VQ_TRAINING = {"learning_rate": 1e-4, "weight_decay": 0.0, "reg_type": "vq", "recon_type": "l1",
                    "perceptual_weight": 0.0, "gan_weight": 0.0, "codebook_weight": 1.0}
HBM_TBPS = 8.0   # MI355X HBM3E peak (MI355X_MICROARCH.md)
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


def _windows(arms, steps, repeats, warmup=3):
    """ms per call of every arm: ``warmup`` calls each, then ``repeats`` windows per arm, alternating, each
    ``steps`` calls between two HIP events after a device synchronise."""
    import torch
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / steps)
    return ms


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def _emit(rec, out):
    line = json.dumps(rec)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def bench_vq(a, qt):
    """``VAETrainStep.step`` of the LDCT VQVAE against ``vq_forward`` (the same forward without a tape; for the EMA
    codebook in eval mode, since the inference forward refuses a training-mode EMA quantizer)."""
    import torch
    from fmdiff.models.vae import VQVAE
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime.vae_engine import get_vae_engine
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = VQVAE(quantizer_type=qt, **LDCT_VQ).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(3)
    img = torch.rand(a.batch, 1, 256, 256, device="cuda", generator=g)
    step = VAETrainStep(vae, LDCT_VQ_TRAINING, {"latent_type": "vq"})
    eng = get_vae_engine(vae)
    xin = vae.image_to_model_range(img)

    cb = vae.codebook

    def forward():   # only the quantizer reads the flag (dropout is 0): one attribute, not a walk over the modules
        cb.training = False
        eng.vq_forward(xin)
        cb.training = True

    arms = {"step": lambda: step.step(img), "forward": forward}
    ms = _windows(arms, a.steps, a.repeats)
    out = step.step(img)
    launches = {k: _launches(fn) for k, fn in arms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    _emit(dict(workload=f"VQVAE (LDCT_vqvae{'_original' if qt == 'classic' else ''}, {qt} codebook) train step, "
                        f"256x256, batch {a.batch}, eager",
               params=sum(p.numel() for p in vae.parameters()), steps_per_window=a.steps, windows=a.repeats,
               step_ms=_stat(ms["step"]), forward_ms=_stat(ms["forward"]),
               step_to_forward=med["step"] / med["forward"], launches=launches, loss_after=float(out["loss"]),
               vq_after=float(out["vq"]), global_step=step.global_step), a.out)


def bench_gan(a):
    """``VAETrainStep.step`` of the LDCT_magvit_vqvae model block (the LDCT VQVAE with the EMA codebook) with a
    ``MagvitDiscriminatorND(1)`` and gan_weight 0.5 active, beside the same step without the discriminator."""
    import torch
    from fmdiff.models.vae import VQVAE
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    g = torch.Generator(device="cuda").manual_seed(3)
    img = torch.rand(a.batch, 1, 256, 256, device="cuda", generator=g)
    steps = {}
    for key, gw in (("gan_step", 0.5), ("plain_step", 0.0)):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vae = VQVAE(quantizer_type="ema", discriminator_type="magvit", **LDCT_VQ).cuda().train()
        disc = vae.make_discriminator().cuda() if gw else None
        steps[key] = VAETrainStep(vae, dict(LDCT_VQ_TRAINING, gan_weight=gw), {"latent_type": "vq"},
                                  discriminator=disc)
    arms = {k: (lambda st=st: st.step(img)) for k, st in steps.items()}
    ms = _windows(arms, a.steps, a.repeats)
    out = steps["gan_step"].step(img)
    launches = {k: _launches(fn) for k, fn in arms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    _emit(dict(workload=f"VQVAE (LDCT_magvit_vqvae, ema codebook) + MagvitDiscriminatorND(1) adversarial train step, "
                        f"gan_weight 0.5, 256x256, batch {a.batch}, eager",
               disc_params=sum(p.numel() for p in steps["gan_step"].disc.parameters()),
               steps_per_window=a.steps, windows=a.repeats, gan_step_ms=_stat(ms["gan_step"]),
               plain_step_ms=_stat(ms["plain_step"]), gan_to_plain=med["gan_step"] / med["plain_step"],
               launches=launches, loss_after=float(out["loss"]), g_gan_after=float(out["g_gan"]),
               d_gan_after=float(out["d_gan"]), disc_step=steps["gan_step"].disc_step), a.out)


def bench_perc(a):
    """The perceptual term: alone (forward + backward to the image), in the AutoencoderKL step, and its conv plan."""
    import torch
    from fmdiff.models.vae import AutoencoderKL
    from fmdiff.nn.losses import VGGPerceptualLoss
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime.perc_engine import get_perc_engine
    torch.manual_seed(0)
    P = VGGPerceptualLoss(resize=True).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    img8 = torch.rand(8, 1, 256, 256, device="cuda", generator=g)
    rec8 = (img8 + 0.1 * torch.randn(img8.shape, device="cuda", generator=g)).clamp(0, 1)
    plans = []
    with torch.no_grad():
        get_perc_engine(P).forward(rec8, img8, plan_out=plans)
    names = {1: "igemm", 2: "halo8", 3: "halo9"}
    table = [dict(conv=i, out=list(shape), kernel=names.get(pl.kernel, pl.kernel), tile_rows=pl.tile_rows, bco=pl.bco,
                  bpx=pl.bpx, splits=sp) for i, shape, pl, sp in plans]

    def alone():
        r = rec8.clone().requires_grad_()
        P(r, img8).backward()

    def forward_only():
        with torch.no_grad():
            P(rec8, img8)

    img = torch.rand(a.batch, 1, 256, 256, device="cuda", generator=g)
    eps = torch.randn(a.batch, 4, 32, 32, device="cuda", generator=g)
    steps = {}
    for key, w in (("perc_step", 1.0), ("plain_step", 0.0)):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            vae = AutoencoderKL(**LDCT_VAE).cuda()
        steps[key] = VAETrainStep(vae, dict(LDCT_TRAINING, perceptual_weight=w), perceptual=P if w else None)
    arms = {"perc_fwd_bwd_b8": alone, "perc_fwd_b8": forward_only}
    arms.update({k: (lambda st=st: st.step(img, eps)) for k, st in steps.items()})
    ms = _windows(arms, a.steps, a.repeats)
    out = steps["perc_step"].step(img, eps)
    launches = {k: _launches(fn) for k, fn in arms.items()}
    _emit(dict(workload=f"VGGPerceptualLoss (VGG16 widths, random weights, 1x256x256 -> 224x224): alone at batch 8; in "
                        f"the AutoencoderKL (LDCT_autoencoder_kl) train step at batch {a.batch}, eager",
               steps_per_window=a.steps, windows=a.repeats, ms={k: _stat(v) for k, v in ms.items()},
               launches=launches, loss_after=float(out["loss"]), perceptual_after=float(out["perceptual"]),
               conv_plan=table), a.out)


def bench_join(a):
    """``ops.vq_join_bwd`` (fp32 g, the engine's arm, and bf16 g) against the four passes it replaces on the bf16
    data gradient: upcast to fp32, ``ops.vq_backward``, cast to bf16 (the 1x1 data gradient's own bf16 store is
    common to both and not timed).  M = batch x 32 x 32 rows, D = 256, both residual modes."""
    import torch
    from fmdiff.runtime import ops
    N, h, w, D, K = a.batch, 32, 32, 256, 16384
    M = N * h * w
    g = torch.Generator(device="cuda").manual_seed(5)
    e = torch.randn((K, D), device="cuda", generator=g)
    codes = torch.randint(0, K, (N, h, w), device="cuda", generator=g)
    z = e[codes] + 0.3 * torch.randn((N, h, w, D), device="cuda", generator=g)
    g32 = 0.1 * torch.randn((N, h, w, D), device="cuda", generator=g)
    gbf = g32.to(torch.bfloat16)
    gl = torch.full((1,), 0.37, device="cuda")
    r = ops.vq_residual(z, D, codes, e)
    dz32 = torch.empty_like(z)
    out = torch.empty((N, h, w, D), device="cuda", dtype=torch.bfloat16)

    def four(zz, cc, ee):
        return lambda: ops.vq_backward(zz, D, cc, ee, gbf.float(), gl, 0.25, out=dz32).to(torch.bfloat16)

    arms = {"join_f32_codebook": lambda: ops.vq_join_bwd(g32, D, z, codes, e, gl, 0.25, out=out),
            "join_bf16_codebook": lambda: ops.vq_join_bwd(gbf, D, z, codes, e, gl, 0.25, out=out),
            "four_pass_codebook": four(z, codes, e),
            "join_f32_residual": lambda: ops.vq_join_bwd(g32, D, r, None, None, gl, 0.25, out=out),
            "join_bf16_residual": lambda: ops.vq_join_bwd(gbf, D, r, None, None, gl, 0.25, out=out),
            "four_pass_residual": four(r, None, None)}
    assert torch.equal(arms["join_bf16_codebook"](), arms["four_pass_codebook"]())
    per = 1
    if a.graph:   # device time: 50 calls of an arm captured once and replayed, so the host's launch rate drops out
        per = 50
        graphs = {}
        for k, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for _ in range(per):
                    fn()
        arms = {k: gr.replay for k, gr in graphs.items()}
    ms = {k: [t / per for t in v] for k, v in _windows(arms, 50 * a.steps // per, a.repeats).items()}
    # bytes a join moves per row: g (4 or 2 D) + z or the residual (4 D) [+ the code row (4 D) + the code (8)] + out (2 D)
    by = {"join_f32_codebook": M * (4 * D + 4 * D + 4 * D + 8 + 2 * D), "join_bf16_codebook": M * (2 * D + 8 * D + 8 + 2 * D),
          "join_f32_residual": M * (4 * D + 4 * D + 2 * D), "join_bf16_residual": M * (2 * D + 4 * D + 2 * D)}
    rec = dict(workload=f"latent join, M = {M} rows, D = {D}, K = {K}" + (", graph replay" if a.graph else ", eager"),
               calls_per_window=50 * a.steps, windows=a.repeats,
               us={k: {kk: 1e3 * vv for kk, vv in _stat(v).items()} for k, v in ms.items()})
    rec["tb_per_s"] = {k: by[k] / (1e-3 * statistics.median(ms[k])) / 1e12 for k in by}
    rec["hbm_frac"] = {k: v / HBM_TBPS for k, v in rec["tb_per_s"].items()}
    rec["four_pass_over_join"] = {m: statistics.median(ms[f"four_pass_{m}"]) / statistics.median(ms[f"join_bf16_{m}"])
                                  for m in ("codebook", "residual")}
    _emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph", action="store_true",
                    help="join arm: time replays of a captured graph of 50 calls (device time) instead of eager calls")
    ap.add_argument("--arm", default="kl", choices=("kl", "vq_ema", "vq_classic", "join", "gan", "perc", "all"))
    ap.add_argument("--perceptual", action="store_true", help="also run the perceptual-term arm (--arm perc)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_vae_train needs a ROCm GPU"
    torch.cuda.set_stream(torch.cuda.Stream())
    if a.arm in ("kl", "all"):
        bench_kl(a)
    if a.arm in ("vq_ema", "all"):
        bench_vq(a, "ema")
    if a.arm in ("vq_classic", "all"):
        bench_vq(a, "classic")
    if a.arm in ("gan", "all"):
        bench_gan(a)
    if a.arm in ("perc", "all") or a.perceptual:
        bench_perc(a)
    if a.arm in ("join", "all"):
        bench_join(a)


def bench_kl(a):
    import torch
    from fmdiff.models.vae import AutoencoderKL
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime.vae_engine import get_vae_engine
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
    ms = _windows(arms, a.steps, a.repeats)
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
    _emit(rec, a.out)


if __name__ == "__main__":
    main()
