"""VAE trainer pieces (reference ``src/pipelines/train/vae_lib.py``): the scheduler factory, the discriminator
gate and the training criterion as one object over the HIP loss kernels (``fmdiff.nn.losses.vae``,
``csrc/vae_loss.hip``), and one whole AutoencoderKL or VQVAE optimizer step on the engine (``VAETrainStep``),
with or without the adversarial half (a discriminator of ``fmdiff.nn.modules.vae.discriminators``) and the perceptual
term (``fmdiff.nn.losses.VGGPerceptualLoss``), with gradient accumulation over micro-batches and a validation pass
(``VAETrainStep.evaluate``).  ``train`` is the reference's loop around them: epochs, validation, the out-of-memory
policy, checkpoints, ``metrics.csv`` and pictures; dataset readers are out of scope."""
from __future__ import annotations

import logging
import math
from pathlib import Path
from typing import Any, Dict, Optional

import torch

from ... import utils as U
from ...nn.losses.vae import discriminator_hinge_loss, generator_hinge_loss, recon_loss

__all__ = ["VAECriterion", "VAETrainStep", "train", "debug_visual_only", "next_micro_batch", "metrics_keys",
           "epoch_order"]

_log = logging.getLogger(__name__)

TOTALS_KEYS = ("loss", "recon", "kl", "perceptual", "g_gan", "d_gan", "vq")


def _make_scheduler(optimizer: torch.optim.Optimizer, cfg: Dict[str, Any]):
    from torch.optim.lr_scheduler import CosineAnnealingLR, ExponentialLR, StepLR
    sched_cfg = cfg.get("scheduler")
    if not sched_cfg:
        return None
    name = (sched_cfg.get("name") or "").lower()
    params = sched_cfg.get("params", {})
    if name == "steplr":
        return StepLR(optimizer, **params)
    if name == "cosineannealinglr":
        return CosineAnnealingLR(optimizer, **params)
    if name == "exponentiallr":
        return ExponentialLR(optimizer, **params)
    if name == "":
        return None
    raise ValueError(f"Unsupported scheduler '{name}'.")


def _disc_is_active(discriminator, gan_weight: float, gan_start: int, gan_start_steps: Optional[int], epoch: int,
                    global_step: int) -> bool:
    if discriminator is None or gan_weight <= 0:
        return False
    if gan_start_steps is not None:
        return global_step >= gan_start_steps
    return epoch >= gan_start


class VAECriterion:
    """The loss composition of the reference trainer (``vae_lib.py:226-275``) from the same config keys and
    defaults::

        total = recon + kl_scale(step) * kl.mean() + effective_codebook_weight * vq_loss
                + perceptual_weight * perceptual + gan_weight * g_gan

    ``recon`` is ``recon_loss(rec, target, recon_type)``; ``kl`` the per-sample KL of ``reparameterize_kl`` /
    ``VAEEngine.kl_forward``; ``vq_loss`` the quantizer's; ``perceptual`` the ``VGGPerceptualLoss`` of the reconstructed image against the target
    (``perceptual_weight > 0`` needs the ``perceptual=`` module at construction and refuses without it);
    ``g_gan = generator_hinge_loss(fake_pred)``.  A call
    returns the parts as a dict of device scalars under the reference's ``totals`` keys (absent parts are a device
    zero); ``out["loss"]`` carries the gradient.  Nothing in it synchronises with the host: ``global_step`` is a
    host integer that only selects the host-side ``kl_scale`` factor."""

    def __init__(self, training_cfg: Dict[str, Any], model_cfg: Optional[Dict[str, Any]] = None, *,
                 perceptual=None) -> None:
        model_cfg = model_cfg or {}
        self.perceptual = perceptual
        self.reg_type = str(training_cfg.get("reg_type", "kl")).lower()
        self.recon_type = training_cfg.get("recon_type", "l1")
        self.perceptual_weight = float(training_cfg.get("perceptual_weight", 0.0))
        self.gan_weight = float(training_cfg.get("gan_weight", 0.0))
        self.gan_start = int(training_cfg.get("gan_start", 0))
        gss = training_cfg.get("gan_start_steps")
        self.gan_start_steps = None if gss is None else int(gss)
        self.kl_weight = float(training_cfg.get("kl_weight", 0.0))
        self.kl_anneal_steps = int(training_cfg.get("kl_anneal_steps", 0))
        self.codebook_weight = float(training_cfg.get("codebook_weight", 1.0))
        self.latent_type = str(model_cfg.get("latent_type", "kl")).lower()
        codebook_active = self.latent_type == "vq" or self.reg_type == "vq"
        self.effective_codebook_weight = self.codebook_weight if codebook_active else 0.0
        if self.perceptual_weight > 0 and perceptual is None:
            raise NotImplementedError("perceptual_weight > 0 needs the perceptual module: pass perceptual= (a "
                                      "fmdiff.nn.losses.VGGPerceptualLoss with its weights loaded), or set "
                                      "perceptual_weight to 0")
        if str(self.recon_type) not in ("l1", "mse", "bce", "focal", "bce_focal"):
            raise ValueError(f"Unsupported recon_type '{self.recon_type}'.")
        self._zero: Dict[str, torch.Tensor] = {}

    def kl_scale(self, global_step: int) -> float:
        kl_scale = self.kl_weight
        if self.kl_anneal_steps > 0:
            step_for_anneal = max(1, global_step + 1)
            kl_scale = self.kl_weight * min(1.0, step_for_anneal / max(1, self.kl_anneal_steps))
        return kl_scale

    def disc_is_active(self, discriminator, epoch: int, global_step: int) -> bool:
        return _disc_is_active(discriminator, self.gan_weight, self.gan_start, self.gan_start_steps, epoch,
                               global_step)

    def _z(self, dev) -> torch.Tensor:
        key = str(dev)
        if key not in self._zero:
            self._zero[key] = torch.zeros((), device=dev, dtype=torch.float32)
        return self._zero[key]

    def __call__(self, rec: torch.Tensor, target: torch.Tensor, *, kl: Optional[torch.Tensor] = None,
                 vq_loss: Optional[torch.Tensor] = None, fake_pred: Optional[torch.Tensor] = None,
                 perceptual: Optional[torch.Tensor] = None, global_step: int = 0, channels: Optional[int] = None,
                 grad_bf16: Optional[list] = None) -> Dict[str, torch.Tensor]:
        """``rec``: the raw decoder output (channels-first, or with ``channels=C`` the head's channels-last
        output read in place); ``target``: the image in [0, 1], channels-first.  ``fake_pred``: the
        discriminator's logits on the reconstruction when it is active.  ``perceptual``: the perceptual term of
        this batch (a device scalar, ``VGGPerceptualLoss.forward_image(rec, image_map, target)``)."""
        zero = self._z(rec.device)
        recon = recon_loss(rec, target, self.recon_type, channels=channels, grad_bf16=grad_bf16)
        total = recon
        kl_term = zero
        if kl is not None:
            kl_term = kl.mean()
            total = total + self.kl_scale(global_step) * kl_term
        vq = zero
        if vq_loss is not None:
            vq = vq_loss
            total = total + self.effective_codebook_weight * vq
        perc = zero
        if perceptual is not None:
            if self.perceptual is None:
                raise ValueError("VAECriterion: a perceptual term needs perceptual= at construction")
            perc = perceptual
            total = total + self.perceptual_weight * perc
        g_gan = zero
        if fake_pred is not None:
            g_gan = generator_hinge_loss(fake_pred)
            total = total + self.gan_weight * g_gan
        return {"loss": total, "recon": recon.detach(), "kl": kl_term.detach(), "perceptual": perc.detach(),
                "g_gan": g_gan.detach(), "d_gan": zero, "vq": vq.detach()}

    def discriminator_loss(self, real_pred: torch.Tensor, fake_pred: torch.Tensor) -> torch.Tensor:
        """``d_gan``: the hinge loss of the discriminator on real and (detached) reconstructed images."""
        return discriminator_hinge_loss(real_pred, fake_pred)


class VAETrainStep:
    """One optimizer step of AutoencoderKL or VQVAE on the engine, the body of the reference's loop
    (``vae_lib.py:198-316``) without AMP, and its validation body (``evaluate``); the adversarial half runs when a ``discriminator`` is
    given and active, the perceptual term when ``perceptual`` is given and ``perceptual_weight > 0`` (see
    ``step``)::

        inputs = model.image_to_model_range(raw_images)
        rec, z, kl = model.forward_train(inputs, eps)
        out = VAECriterion(...)(rec, raw_images, kl=kl, global_step=global_step)
        out["loss"].backward()
        AdamW(lr, weight_decay)                      # torch defaults otherwise, as the reference builds it

    A model with a codebook takes the VQ path: ``rec, aux = model.forward_train(inputs)`` and
    ``criterion(rec, raw_images, vq_loss=aux["vq_loss"], global_step=global_step)``; it has no posterior noise
    (``eps`` raises).  The EMA codebook's buffers are updated by that forward, as in the reference, and are not
    optimizer state.  The classic ``codebook.embedding`` is a Parameter that receives no gradient in the
    reference, so torch's AdamW skips it, weight decay included: here it is kept out of the flat update (it is
    laid out behind the trained parameters and the AdamW launch stops short of it), so it stays bit-identical for
    any ``weight_decay``.

    Parameters, gradients and Adam moments are flat fp32 buffers, all owned by ``FlatParams`` (``flat``, and
    ``disc_flat`` for the discriminator), which also writes and reads the torch optimizer state; the optimizer is one
    ``ops.adamw`` launch, and because it writes the parameters through raw pointers the step then re-derives the
    engine's bf16 weight layouts and the folded quant_conv.  ``global_step`` is a host integer used for
    ``kl_scale`` and Adam's bias correction only; nothing in ``step`` synchronises with the host."""

    def __init__(self, model, training_cfg: Dict[str, Any], model_cfg: Optional[Dict[str, Any]] = None, *,
                 discriminator=None, disc_grad_from_generator: bool = True, perceptual=None,
                 lr: Optional[float] = None, weight_decay: Optional[float] = None, betas=(0.9, 0.999),
                 eps: float = 1e-8) -> None:
        from ...runtime.vae_engine import get_vae_engine
        from .fused import FlatParams
        self.criterion = VAECriterion(training_cfg, model_cfg, perceptual=perceptual)
        if perceptual is not None:
            if training_cfg.get("use_amp"):
                raise NotImplementedError("VAETrainStep with a perceptual module: use_amp (AMP / GradScaler) is not "
                                          "built")
            if training_cfg.get("perceptual_device") is not None:
                raise NotImplementedError("VAETrainStep: perceptual_device (a perceptual module on another device) "
                                          "is not built")
        if self.criterion.gan_weight > 0 and discriminator is None:
            raise NotImplementedError("gan_weight > 0 needs a discriminator: pass discriminator= (a "
                                      "MagvitDiscriminatorND or PatchGANDiscriminatorND of "
                                      "fmdiff.nn.modules.vae.discriminators), or set gan_weight to 0")
        if discriminator is not None:
            if training_cfg.get("use_amp"):
                raise NotImplementedError("VAETrainStep with a discriminator: use_amp (AMP / GradScaler) is not built")
            if training_cfg.get("disc_device") is not None:
                raise NotImplementedError("VAETrainStep: disc_device (a discriminator on another device) is not built")
        self.vq = hasattr(model, "codebook")
        if self.criterion.effective_codebook_weight != 0.0 and not self.vq:
            raise NotImplementedError("VAETrainStep: a codebook weight needs a model with a codebook (VQVAE); "
                                      "AutoencoderKL trains with latent_type / reg_type 'kl'")
        self.model = model
        self.eng = get_vae_engine(model)
        self.eng.check_trainable()
        self.lr = float(training_cfg.get("learning_rate", 1e-4) if lr is None else lr)
        self.weight_decay = float(training_cfg.get("weight_decay", 0.0) if weight_decay is None else weight_decay)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        # parameters that get no gradient in the reference (the classic codebook) behind the trained ones
        frozen = [p for p in model.codebook.parameters()] if self.vq else []
        ids = {id(p) for p in frozen}
        self.flat = FlatParams(model, first=[p for p in model.parameters() if id(p) not in ids] if frozen else None)
        self.n_trained = self.flat.split_at if frozen else self.flat.numel
        self.m, self.v = self.flat.m, self.flat.v   # the same tensors: the flat object owns them
        self.global_step = 0
        self.eng.invalidate_weights()   # the parameters moved into the flat buffer
        self.disc = discriminator
        self.disc_grad_from_generator = bool(disc_grad_from_generator)
        if discriminator is not None:
            from ...runtime.disc_engine import get_disc_engine
            out_ch = model.decoder.conv_out.conv.out_channels
            if discriminator.in_channels != out_ch:
                raise ValueError(f"VAETrainStep: the discriminator reads {discriminator.in_channels} channels, the "
                                 f"decoder writes {out_ch}")
            discriminator.train()          # as the reference's loop does at the start of every epoch
            self.disc_eng = get_disc_engine(discriminator)
            self.disc_flat = FlatParams(discriminator)
            self.disc_m, self.disc_v = self.disc_flat.m, self.disc_flat.v
            self.disc_step = 0             # Adam's count: active steps only (torch skips parameters without a grad)
            dlr = training_cfg.get("disc_lr")
            self.disc_lr = self.lr if dlr is None else float(dlr)
            self.disc_weight_decay = 0.01  # torch.optim.AdamW's default, as the reference builds the optimizer
            self.disc_eng.invalidate_weights()
        rt = str(self.criterion.recon_type).lower()
        self.image_map = "sigmoid" if rt in ("bce", "focal", "bce_focal") else "clamp"   # raw_output_to_image
        self.perc = perceptual if self.criterion.perceptual_weight > 0 else None   # weight 0: never called
        if self.perc is not None:
            out_ch = model.decoder.conv_out.conv.out_channels
            if out_ch not in (1, 3):
                raise ValueError(f"VAETrainStep: the perceptual loss reads 1 or 3 channels, the decoder writes {out_ch}")
            self.perc.eval()

    def step(self, raw_images: torch.Tensor, eps: Optional[torch.Tensor] = None, epoch: int = 0,
             micro_batch: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """``raw_images``: the batch in [0, 1], NCHW fp32 on the device; ``eps``: the posterior noise (None: drawn
        on the device; a VQVAE takes none); ``epoch``: the reference's epoch number, read by the discriminator gate
        only.  Returns VAECriterion's totals as device scalars (``loss`` detached).

        ``micro_batch`` smaller than the batch: gradient accumulation as the reference does it
        (``vae_lib.py:206-316``).  Both gradient buffers are zeroed once, the batch (and ``eps``) is split with
        ``split(micro_batch)``, every chunk runs the body below with ``(loss / accum).backward()`` and
        ``(d_gan / accum).backward()``, ``accum`` the number of chunks (not the chunk's share of the batch, so
        unequal chunks are not the full-batch mean: the reference's arithmetic), and then ``global_step`` advances
        once and each network gets one AdamW launch.  ``kl_scale`` and the discriminator gate read the same
        ``global_step`` for every chunk; the EMA codebook and BatchNorm's running statistics move once per chunk, as
        the reference's forwards move them.  The returned values are then the sample-weighted means
        ``sum_c value_c n_c / N``, so that ``total += out * N`` gives the reference's ``totals``.

        An exception inside the step leaves the object usable: what the engines keep between forward and backward is
        dropped before it propagates, and ``global_step``, the moments and the parameters have not moved (the EMA
        and BatchNorm buffers may have, as in the reference).

        With a discriminator that is active at this step (``VAECriterion.disc_is_active``) the body is the
        reference's (``vae_lib.py:248-316``): ``fake_pred = D(image(rec))`` enters the criterion, and its backward
        reaches the VAE through the discriminator's data gradients and, as in the reference (which zeroes the
        discriminator's gradients only at the start of the batch), also leaves ``gan_weight * d g_gan / d theta_D`` in
        the discriminator's gradients (``disc_grad_from_generator=False``: that weight-gradient work is skipped);
        then ``d_gan = discriminator_hinge_loss(D(raw_images), D(image(rec).detach()))`` and its backward; one AdamW
        launch per network.  An inactive step is the step without a discriminator and leaves it untouched.

        With a perceptual module and ``perceptual_weight > 0`` the criterion also receives
        ``perceptual.forward_image(rec, image_map, raw_images)`` (``vae_lib.py:241-246``), whose backward adds the
        data gradient of the frozen stack to that of the other terms; the module itself is never changed."""
        if self.vq and eps is not None:
            raise ValueError("VAETrainStep.step: eps is the AutoencoderKL posterior noise; a VQVAE has none")
        N = raw_images.shape[0]
        if micro_batch is not None and int(micro_batch) < 1:
            raise ValueError(f"VAETrainStep.step: micro_batch must be at least 1, got {micro_batch}")
        active = self.disc is not None and self.criterion.disc_is_active(self.disc, epoch, self.global_step)
        self.flat.grad.zero_()
        if active:
            self.disc_flat.grad.zero_()
        try:
            if micro_batch is None or int(micro_batch) >= N:
                out = self._chunk(raw_images, eps, active, 1)
            else:
                chunks = raw_images.split(int(micro_batch))
                eps_chunks = [None] * len(chunks) if eps is None else eps.split(int(micro_batch))
                outs = [self._chunk(c, e, active, len(chunks)) for c, e in zip(chunks, eps_chunks)]
                out = _weighted_mean(outs, [c.shape[0] for c in chunks])
        except BaseException:
            self._drop_saved_state()
            raise
        self.global_step += 1
        from ...runtime import ops
        f, n = self.flat, self.n_trained
        ops.adamw(f.data[:n], f.grad[:n], self.m[:n], self.v[:n], self.lr, self.betas[0], self.betas[1], self.eps,
                  self.weight_decay, self.global_step)
        self.eng.invalidate_weights()
        if active:
            self.disc_step += 1
            d = self.disc_flat
            ops.adamw(d.data, d.grad, self.disc_m, self.disc_v, self.disc_lr, self.betas[0], self.betas[1], self.eps,
                      self.disc_weight_decay, self.disc_step)
            self.disc_eng.invalidate_weights()
        return out

    def _chunk(self, raw_images, eps, active: bool, accum: int) -> Dict[str, torch.Tensor]:
        """Forward, criterion and backward of one chunk; with ``accum > 1`` the losses are divided by it before
        their backward.  The gradients accumulate into the flat buffers."""
        rec = kw = out = None
        try:
            inputs = self.model.image_to_model_range(raw_images)
            if self.vq:
                rec, aux = self.model.forward_train(inputs)
                kw = dict(vq_loss=aux["vq_loss"])
            else:
                rec, _, kl = self.model.forward_train(inputs, eps, sample_posterior=True)
                kw = dict(kl=kl)
            if active:
                kw["fake_pred"] = self.disc.forward_image(rec, self.image_map,
                                                          param_grads=self.disc_grad_from_generator)
            if self.perc is not None:
                kw["perceptual"] = self.perc.forward_image(rec, self.image_map, raw_images)
            out = self.criterion(rec, raw_images, global_step=self.global_step, **kw)
            (out["loss"] if accum == 1 else out["loss"] / accum).backward()
            out["loss"] = out["loss"].detach()
            if active:
                real_pred = self.disc(raw_images.detach())
                fake_pred_detached = self.disc.forward_image(rec.detach(), self.image_map)
                d_gan = self.criterion.discriminator_loss(real_pred, fake_pred_detached)
                if accum == 1:
                    d_gan.backward()
                else:
                    # This backward runs the discriminator's two passes (real, fake), and each adds into .grad on its
                    # own.  Autograd sums the contributions of one backward before it accumulates, so across chunks
                    # the reference adds (real + fake) / accum as one term: sum them apart from what earlier chunks
                    # left, then add once (two equal chunks then give the full batch's bits).
                    held = self.disc_flat.grad.clone()
                    self.disc_flat.grad.zero_()
                    (d_gan / accum).backward()
                    self.disc_flat.grad.add_(held)
                out["d_gan"] = d_gan.detach()
            return out
        except BaseException:
            rec = kw = out = aux = kl = None   # the autograd graph of this chunk, with the tapes its nodes hold
            raise

    def _drop_saved_state(self) -> None:
        """After a failed step: nothing of it is left on the engines for the next one (the backward slot of the
        head, queued weight gradients, a partial gradient of the folded conv_out)."""
        engines = [self.eng]
        if self.disc is not None:
            engines.append(self.disc_eng)
        if self.perc is not None:
            from ...runtime.perc_engine import get_perc_engine
            engines.append(get_perc_engine(self.perc))
        for e in engines:
            e.drop_saved_state()
        fold = self.eng._fold
        if fold is not None:
            for p in (fold.weight, fold.bias):
                if p.grad is not None:
                    p.grad.zero_()

    @torch.no_grad()
    def evaluate(self, raw_images: torch.Tensor, epoch: int = 0,
                 micro_batch: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """The validation body of the reference (``vae_lib.py:381-455``) for one batch: model and discriminator in
        ``eval()``, no gradient.  AutoencoderKL decodes the posterior's mode (``model(x, sample_posterior=False)``)
        with ``kl = posterior.kl().mean()``; a VQVAE runs ``model(x)`` with its codebook frozen (no EMA update in
        eval mode).  Reconstruction, perceptual and ``kl_scale`` arithmetic are the training step's (the same
        ``VAECriterion`` at the current ``global_step``); with an active discriminator ``g_gan`` comes from
        ``D(image(rec))`` and ``d_gan = discriminator_hinge_loss(D(raw), D(image(rec)))``, BatchNorm on its running
        statistics.  Chunks (``split(micro_batch)``) and the sample-weighted means are as in ``step``.

        Nothing is changed: no parameter, gradient, moment, ``global_step``, running statistic or EMA buffer; the
        modules come back in the mode they were in."""
        if micro_batch is not None and int(micro_batch) < 1:
            raise ValueError(f"VAETrainStep.evaluate: micro_batch must be at least 1, got {micro_batch}")
        active = self.disc is not None and self.criterion.disc_is_active(self.disc, epoch, self.global_step)
        modules = [self.model] + ([self.disc] if self.disc is not None else [])
        modes = [m.training for m in modules]
        for m in modules:
            m.eval()
        try:
            N = raw_images.shape[0]
            chunks = raw_images.split(N if micro_batch is None else min(int(micro_batch), N)) if N else (raw_images,)
            outs = []
            for raw in chunks:
                inputs = self.model.image_to_model_range(raw)
                if self.vq:
                    rec, aux = self.model(inputs)
                    kw = dict(vq_loss=aux["vq_loss"])
                else:
                    rec, posterior = self.model(inputs, sample_posterior=False)
                    kw = dict(kl=posterior.kl())
                if active:
                    kw["fake_pred"] = self.disc.forward_image(rec, self.image_map)
                if self.perc is not None:
                    kw["perceptual"] = self.perc.forward_image(rec, self.image_map, raw)
                out = self.criterion(rec, raw, global_step=self.global_step, **kw)
                if active:
                    out["d_gan"] = self.criterion.discriminator_loss(self.disc(raw), kw["fake_pred"])
                outs.append(out)
        finally:
            for m, was in zip(modules, modes):
                m.train(was)
        return outs[0] if len(outs) == 1 else _weighted_mean(outs, [c.shape[0] for c in chunks])

    def disc_state_dict(self) -> Dict[str, Any]:
        """The discriminator optimizer's state in ``torch.optim.AdamW.state_dict()`` form (state keyed by the index
        in ``discriminator.parameters()``)."""
        if self.disc is None:
            raise RuntimeError("VAETrainStep.disc_state_dict: no discriminator")
        return self.disc_flat.adamw_state_dict(self.disc_step, lr=self.disc_lr, betas=self.betas, eps=self.eps,
                                               weight_decay=self.disc_weight_decay)

    def load_disc_state_dict(self, sd: Dict[str, Any]) -> None:
        """Inverse of ``disc_state_dict`` (also takes a torch AdamW state of the same discriminator)."""
        if self.disc is None:
            raise RuntimeError("VAETrainStep.load_disc_state_dict: no discriminator")
        self.disc_step = self.disc_flat.load_adamw_state_dict(sd)
        groups = sd.get("param_groups") or []
        if groups:
            self.disc_lr = float(groups[0].get("lr", self.disc_lr))
            self.disc_weight_decay = float(groups[0].get("weight_decay", self.disc_weight_decay))

    def state_dict(self) -> Dict[str, Any]:
        """The optimizer state in ``torch.optim.AdamW.state_dict()`` form (state keyed by the index in
        ``model.parameters()``) plus ``global_step``."""
        sd = self.flat.adamw_state_dict(self.global_step, lr=self.lr, betas=self.betas, eps=self.eps,
                                        weight_decay=self.weight_decay)
        sd["global_step"] = self.global_step
        return sd

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Inverse of ``state_dict`` (also takes a torch AdamW state of the same model)."""
        steps = self.flat.load_adamw_state_dict(sd)
        self.global_step = int(sd.get("global_step", steps))
        groups = sd.get("param_groups") or []
        if groups:
            g = groups[0]
            self.lr = float(g.get("lr", self.lr))
            self.weight_decay = float(g.get("weight_decay", self.weight_decay))
            self.betas = tuple(float(b) for b in g.get("betas", self.betas))
            self.eps = float(g.get("eps", self.eps))


def _weighted_mean(outs, sizes) -> Dict[str, torch.Tensor]:
    """``sum_c value_c n_c / N`` for every key of the chunks' totals, in chunk order, as fp32 device scalars."""
    total = sum(sizes)
    res = {}
    for k in outs[0]:
        acc = outs[0][k] * sizes[0]
        for o, n in zip(outs[1:], sizes[1:]):
            acc = acc + o[k] * n
        res[k] = acc / total
    return res


# ---------------------------------------------------------------------------------------------------- the loop
OOM_DISABLED_MESSAGE = ("The current batch size is too large, please set it to a lower value or enable "
                        "microbatching.")


def is_out_of_memory(err: BaseException) -> bool:
    return isinstance(err, RuntimeError) and "out of memory" in str(err).lower()


def next_micro_batch(current: int, allow_microbatching: bool, err: Optional[BaseException] = None) -> int:
    """The reference's answer to an out-of-memory error (``vae_lib.py:347-358``): the micro-batch to retry the batch
    with.  Microbatching disabled: its ``RuntimeError``; nothing left to halve (``current <= 1``): ``err`` again."""
    if not allow_microbatching:
        raise RuntimeError(OOM_DISABLED_MESSAGE) from err
    if current <= 1:
        raise err if err is not None else RuntimeError("out of memory at a micro-batch of 1")
    return max(1, current // 2)


def micro_batch_warning(current_micro: int, batch_size: int) -> str:
    return (f"The maximum batch size for the current configuration is {current_micro}; training with "
            f"{math.ceil(batch_size / current_micro)} micro batches of size {current_micro} for gradient "
            f"accumulation.")


def metrics_keys(training_cfg: Dict[str, Any]) -> list:
    """The columns of ``metrics.csv`` after ``epoch`` (reference ``vae_lib.py:101-110``)."""
    keys = ["loss", "recon"]
    reg_type = str(training_cfg.get("reg_type", "kl")).lower()
    if reg_type == "kl" or float(training_cfg.get("kl_weight", 0.0)) > 0:
        keys.append("kl")
    if reg_type == "vq" or float(training_cfg.get("codebook_weight", 1.0)) > 0:
        keys.append("vq")
    if float(training_cfg.get("perceptual_weight", 0.0)) > 0:
        keys.append("perceptual")
    if float(training_cfg.get("gan_weight", 0.0)) > 0:
        keys.extend(["g_gan", "d_gan"])
    return keys


def metrics_header(training_cfg: Dict[str, Any]) -> str:
    return "epoch," + ",".join(metrics_keys(training_cfg)) + "\n"


def epoch_seed(seed, epoch: int) -> int:
    """The seed of everything that is drawn per epoch outside the training noise stream (the batch order, the
    ``gen`` picture's noise): a function of ``(seed or 0, epoch)`` only."""
    return (int(seed or 0) * 1000003 + int(epoch)) % (2 ** 63 - 1)


def epoch_order(n: int, seed, epoch: int) -> list:
    """The order in which epoch ``epoch`` visits a dataset of ``n`` items."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(epoch_seed(seed, epoch))).tolist()


class _EpochLoader:
    """A shuffling ``DataLoader`` whose sampler draws from a generator of its own, reseeded by ``set_epoch``."""

    def __init__(self, dataset, batch_size: int, num_workers: int, seed, pin_memory: bool) -> None:
        from torch.utils.data import DataLoader, RandomSampler
        self.seed = seed
        self.order_gen, self.worker_gen = torch.Generator(), torch.Generator()
        self.loader = DataLoader(dataset, batch_size=batch_size, sampler=RandomSampler(dataset, generator=self.order_gen),
                                 num_workers=num_workers, pin_memory=pin_memory, generator=self.worker_gen)

    def set_epoch(self, epoch: int) -> None:
        self.order_gen.manual_seed(epoch_seed(self.seed, epoch))
        self.worker_gen.manual_seed(epoch_seed(self.seed, epoch))

    def __iter__(self):
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


def _is_none(v) -> bool:
    return v is None or (isinstance(v, str) and v.lower() == "none")


def _refuse_unbuilt(training_cfg: Dict[str, Any]) -> None:
    if training_cfg.get("use_amp"):
        raise NotImplementedError("vae_lib.train: use_amp (AMP / GradScaler) is not built; set use_amp to false")
    for key in ("disc_device", "perceptual_device"):
        if not _is_none(training_cfg.get(key)):
            raise NotImplementedError(f"vae_lib.train: {key} (a second device) is not built; remove {key}")


def _train_device(training_cfg: Dict[str, Any]) -> torch.device:
    manual = training_cfg.get("manual_device")
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if _is_none(manual) else torch.device(manual)
    if device.type != "cuda":
        raise RuntimeError(f"vae_lib.train: VAE training runs on the HIP engine and has no CPU path (device {device})")
    return U.resolve_device(device, device)


def _build_discriminator(model, device):
    """The reference's choice (``make_discriminator``): MAGVIT for a VQVAE that asks for it, else the PatchGAN."""
    from ...nn.modules.vae.discriminators import PatchGANDiscriminatorND
    if hasattr(model, "codebook") and getattr(model, "discriminator_type", "patchgan") == "magvit":
        return model.make_discriminator().to(device)
    return PatchGANDiscriminatorND(in_channels=model.decoder.conv_out.conv.out_channels, spatial_dims=2).to(device)


def _build_perceptual(training_cfg: Dict[str, Any], perceptual, device):
    if perceptual is not None:
        return perceptual.to(device)
    path = training_cfg.get("perceptual_weights")
    if _is_none(path):
        raise NotImplementedError("vae_lib.train: perceptual_weight > 0 needs the VGG16 weights, and nothing is ever "
                                  "downloaded: pass perceptual= (a fmdiff.nn.losses.VGGPerceptualLoss with its "
                                  "weights loaded) or set training.perceptual_weights to a local torchvision vgg16 "
                                  "state dict")
    from ...nn.losses import VGGPerceptualLoss
    module = VGGPerceptualLoss(resize=True)   # as the reference's trainer builds it
    module.load_vgg_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    return module.to(device)


def _cpu_state(module) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def _reconstruct(model, batch, recon_type):
    """Eval-mode reconstruction of an image batch in [0, 1], back in image space."""
    out = model(model.image_to_model_range(batch)) if hasattr(model, "codebook") else \
        model(model.image_to_model_range(batch), sample_posterior=False)
    return model.raw_output_to_image(out[0], recon_type=recon_type)


def train(dataset, json_path, val_dataset=None, resume=None, *, perceptual=None):
    """The reference's VAE trainer (``vae_lib.py:61-552``), epoch for epoch, on ``VAETrainStep``: 2-D, eager, one
    GPU.  ``dataset`` / ``val_dataset``: items ``{"target": tensor [C, H, W] in [0, 1]}``.  Returns the run
    directory.  What differs from the reference is listed in DESIGN.md section 7."""
    if dataset is None:
        raise NotImplementedError("vae_lib.train: building a dataset from the config is out of scope (DESIGN.md "
                                  "section 7); pass a dataset of {\"target\": tensor} items")
    from torch.utils.data import DataLoader
    from ...utils.model_utils.vae_utils import build_vae_model
    logging.basicConfig(level=logging.INFO, format="%(asctime)s | %(levelname)s | %(message)s", force=True)
    cfg = U.load_json_config(json_path)
    tr = cfg["training"]
    model_cfg = cfg.get("model", {})
    _refuse_unbuilt(tr)
    seed = tr.get("seed")
    U.set_seed(seed)
    device = _train_device(tr)

    batch_size = int(tr.get("batch_size", 4))
    allow_micro = bool(tr.get("allow_microbatching", True))
    num_workers = int(tr.get("num_workers", 4))
    epochs = int(tr.get("epochs", 1))
    recon_type = tr.get("recon_type", "l1")
    save_every = int(tr.get("save_every", 1))
    log_every = max(1, int(tr.get("log_every", 50)))
    base_dir = Path(tr.get("output_dir", "checkpoints/vae"))
    out_dir = U.allocate_run_dir(base_dir) if resume is None else base_dir
    tr["output_dir"] = str(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    if not (out_dir / "train_config.json").exists():
        U.save_json_config(out_dir / "train_config.json", cfg)
    keys = metrics_keys(tr)
    metrics_path = out_dir / "metrics.csv"
    if not metrics_path.exists():
        metrics_path.write_text(metrics_header(tr))

    resume_flag = resume if resume is not None else tr.get("resume")
    if _is_none(resume_flag):
        resume_flag = None
    payload = None
    if resume_flag:
        ckpt_path = Path(resume_flag) if isinstance(resume_flag, str) else U.latest_checkpoint(out_dir)
        if ckpt_path and ckpt_path.exists():
            payload = torch.load(ckpt_path, map_location="cpu", weights_only=True)

    model = build_vae_model(cfg, device, None, set_eval=False)
    discriminator = _build_discriminator(model, device) if float(tr.get("gan_weight", 0.0)) > 0 else None
    perc = _build_perceptual(tr, perceptual, device) if float(tr.get("perceptual_weight", 0.0)) > 0 else None
    if payload is not None:   # before the step moves the parameters into its flat buffers
        model.load_state_dict(payload.get("model", payload))
        if discriminator is not None and payload.get("discriminator"):
            discriminator.load_state_dict(payload["discriminator"])
    model.train()
    step = VAETrainStep(model, tr, model_cfg, discriminator=discriminator, perceptual=perc)
    host_opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=step.lr)   # carries the LR schedule only
    scheduler = _make_scheduler(host_opt, tr)

    best_metric = float("inf")
    start_epoch = 1
    if payload is not None:
        if payload.get("optimizer"):
            step.load_state_dict(payload["optimizer"])
        if discriminator is not None and payload.get("disc_optimizer"):
            step.load_disc_state_dict(payload["disc_optimizer"])
        host_opt.param_groups[0]["lr"] = step.lr
        if scheduler is not None and payload.get("scheduler"):
            scheduler.load_state_dict(payload["scheduler"])
        if payload.get("cuda_rng_state") is not None:
            torch.cuda.set_rng_state(payload["cuda_rng_state"], device)
        best_metric = payload.get("best_metric", best_metric)
        start_epoch = int(payload.get("epoch", 0)) + 1
        _log.info("Resumed from %s (epoch %d)", ckpt_path, start_epoch - 1)

    loader = _EpochLoader(dataset, batch_size, num_workers, seed, pin_memory=True)
    val_loader = None
    if val_dataset is not None:
        val_loader = DataLoader(val_dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers,
                                pin_memory=True)
    _log.info("Data: train_samples=%d%s | batch_size=%d | micro_batching=%s | num_workers=%d | epochs=%d",
              len(dataset), f", val_samples={len(val_dataset)}" if val_dataset is not None else "", batch_size,
              "enabled" if allow_micro else "disabled", num_workers, epochs)

    sample_count = int(tr.get("visual_samples", 20))
    visual_enabled = bool(tr.get("save_images", True))
    visual_every = int(tr.get("save_images_every", 1))
    sample_batch = None
    if visual_enabled:
        sample_batch = U.prepare_eval_batch(val_dataset if val_dataset is not None else dataset, sample_count, device,
                                            seed=seed)
    latent = U.latent_shape(model_cfg) if visual_enabled else None

    def fresh_totals():
        return torch.zeros(len(TOTALS_KEYS), device=device, dtype=torch.float64)

    def add(totals, out, bs):
        totals += torch.stack([out[k] for k in TOTALS_KEYS]).double() * bs

    current_micro = batch_size
    warned_micro = False
    for epoch in range(start_epoch, epochs + 1):
        model.train()
        if discriminator is not None:
            discriminator.train()
        loader.set_epoch(epoch)
        totals, num_samples = fresh_totals(), 0
        for i, batch in enumerate(loader):
            raw = batch["target"].to(device, non_blocking=True)
            bs = raw.shape[0]
            while True:
                try:
                    out = step.step(raw, epoch=epoch, micro_batch=current_micro)
                    break
                except RuntimeError as err:
                    if not is_out_of_memory(err):
                        raise
                    nxt = next_micro_batch(current_micro, allow_micro, err)
                    torch.cuda.empty_cache()
                    current_micro = nxt
            add(totals, out, bs)
            num_samples += bs
            if current_micro < batch_size and not warned_micro:
                _log.warning(micro_batch_warning(current_micro, batch_size))
                warned_micro = True
            if (i + 1) % log_every == 0:
                loss, recon = (totals[:2] / max(1, num_samples)).tolist()
                _log.info("Train %d/%d | batch %d/%d | loss %.4f | recon %.4f", epoch, epochs, i + 1, len(loader),
                          loss, recon)
        averaged = dict(zip(TOTALS_KEYS, (totals / max(1, num_samples)).tolist()))   # the epoch's one host read
        _log.info("Epoch %03d | loss %.6f (recon %.6f, perc %.6f, kl %.6f, vq %.6f, g_gan %.6f, d_gan %.6f)", epoch,
                  *(averaged[k] for k in ("loss", "recon", "perceptual", "kl", "vq", "g_gan", "d_gan")))

        val_avg = None
        if val_loader is not None:
            val_totals, val_samples = fresh_totals(), 0
            for batch in val_loader:
                raw = batch["target"].to(device, non_blocking=True)
                add(val_totals, step.evaluate(raw, epoch=epoch, micro_batch=min(current_micro, batch_size)),
                    raw.shape[0])
                val_samples += raw.shape[0]
            val_avg = dict(zip(TOTALS_KEYS, (val_totals / max(1, val_samples)).tolist()))
            _log.info("Epoch %03d | val_loss %.6f (recon %.6f, perc %.6f, kl %.6f, vq %.6f, g_gan %.6f, d_gan %.6f)",
                      epoch, *(val_avg[k] for k in ("loss", "recon", "perceptual", "kl", "vq", "g_gan", "d_gan")))

        if scheduler is not None:
            host_opt.step()   # no gradient, no update: torch wants an optimizer step before a scheduler step
            scheduler.step()
            step.lr = float(host_opt.param_groups[0]["lr"])

        current_metric = val_avg["loss"] if val_avg is not None else averaged["loss"]
        state = {"model": _cpu_state(model), "optimizer": step.state_dict(),
                 "disc_optimizer": step.disc_state_dict() if discriminator is not None else None,
                 "scheduler": scheduler.state_dict() if scheduler is not None else None, "scaler": None,
                 "epoch": epoch, "best_metric": best_metric,
                 "discriminator": _cpu_state(discriminator) if discriminator is not None else None,
                 "cuda_rng_state": torch.cuda.get_rng_state(device)}
        U.save_checkpoint(state, out_dir / "vae_last.pt")
        if current_metric < best_metric:
            best_metric = current_metric
            state["best_metric"] = best_metric
            U.save_checkpoint(state, out_dir / "vae_best.pt")
            _log.info("New best (%.6f) -> %s", best_metric, out_dir / "vae_best.pt")

        with metrics_path.open("a") as handle:
            handle.write(",".join([f"{epoch}"] + [f"{averaged[k]:.6f}" for k in keys]) + "\n")

        if epoch % save_every == 0 or epoch == epochs:
            epoch_dir = out_dir / "epochs" / f"epoch{epoch:04d}"
            U.save_checkpoint(state, epoch_dir / "epoch.pt")
            _log.info("Saved epoch checkpoint: %s", epoch_dir / "epoch.pt")
            if visual_enabled and (epoch % visual_every == 0 or epoch == epochs):
                model.eval()
                with torch.no_grad():
                    rec_vis = _reconstruct(model, sample_batch, recon_type)
                    # a generator of its own: writing pictures does not move the training noise stream
                    g = torch.Generator(device=device).manual_seed(epoch_seed(seed, epoch))
                    noise = torch.randn((sample_count, *latent), device=device, generator=g)
                    gen_vis = model.raw_output_to_image(model.decode(noise), recon_type=recon_type)
                    grids = [U.make_grid(t, 4, 5) for t in (sample_batch.clamp(0.0, 1.0), rec_vis, gen_vis)]
                for grid, name in zip(grids, ("input.png", "recon.png", "gen.png")):
                    U.save_image(grid, epoch_dir / name)
                model.train()
    return out_dir


def debug_visual_only(dataset, json_path, ckpt_path, *, output_dir=None, visual_samples: int = 10, seed=None):
    """Load a trained VAE checkpoint and write the trainer's picture grids only (reference ``vae_lib.py:555-596``):
    ``grid_input.png``, ``grid_output.png`` and ``grid_target.png`` of ``visual_samples`` items under
    ``output_dir`` (default ``<training.output_dir>/debug_train_like``).  The reference's per-sample files need its
    dataset readers, which are out of scope.  Returns the directory."""
    from ...utils.model_utils.diffusion_utils import select_visual_indices
    from ...utils.model_utils.vae_utils import build_vae_model
    logging.basicConfig(level=logging.INFO, format="%(asctime)s | %(levelname)s | %(message)s", force=True)
    cfg = U.load_json_config(json_path)
    model_type = str(cfg.get("model", {}).get("model_type", "")).lower()
    if model_type != "vae":
        raise ValueError(f"Expected model_type 'vae', got '{model_type}'.")
    tr = cfg["training"]
    seed = seed if seed is not None else tr.get("seed")
    U.set_seed(seed)
    device = _train_device(tr)
    model = build_vae_model(cfg, device, ckpt_path=Path(ckpt_path), set_eval=True)
    out_root = Path(output_dir) if output_dir is not None else \
        Path(tr.get("output_dir", "checkpoints/vae")) / "debug_train_like"
    out_root.mkdir(parents=True, exist_ok=True)
    indices = select_visual_indices(dataset, int(visual_samples), seed=seed)
    batch = torch.stack([dataset[i]["target"] for i in indices], dim=0).to(device)
    with torch.no_grad():
        rec_vis = _reconstruct(model, batch, tr.get("recon_type", "l1")).clamp(0.0, 1.0)
    input_vis = batch.clamp(0.0, 1.0)
    rows = max(1, int(math.sqrt(rec_vis.size(0))))
    cols = max(1, rec_vis.size(0) // rows)
    U.save_image(U.make_grid(input_vis, rows, cols), out_root / "grid_input.png")
    U.save_image(U.make_grid(rec_vis, rows, cols), out_root / "grid_output.png")
    U.save_image(U.make_grid(input_vis, rows, cols), out_root / "grid_target.png")
    _log.info("VAE debug visual-only generation completed for %d samples. Output: %s", len(indices), out_root)
    return out_root
