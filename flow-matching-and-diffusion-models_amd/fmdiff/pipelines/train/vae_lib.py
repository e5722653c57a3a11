"""VAE trainer pieces (reference ``src/pipelines/train/vae_lib.py``): the scheduler factory, the discriminator
gate and the training criterion as one object over the HIP loss kernels (``fmdiff.nn.losses.vae``,
``csrc/vae_loss.hip``), and one whole AutoencoderKL or VQVAE optimizer step on the engine (``VAETrainStep``),
with or without the adversarial half (a discriminator of ``fmdiff.nn.modules.vae.discriminators``) and the perceptual
term (``fmdiff.nn.losses.VGGPerceptualLoss``).  The trainer loop itself is not built: the datasets, checkpoints and
images around the step are missing."""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from ...nn.losses.vae import discriminator_hinge_loss, generator_hinge_loss, recon_loss

__all__ = ["VAECriterion", "VAETrainStep", "train"]

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
    (``vae_lib.py:198-316``) without AMP or microbatching; the adversarial half runs when a ``discriminator`` is
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

    Parameters, gradients and Adam moments are flat fp32 buffers (``FlatParams``), the optimizer is one
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
        self.m = torch.zeros_like(self.flat.data)
        self.v = torch.zeros_like(self.flat.data)
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
            self.disc_m = torch.zeros_like(self.disc_flat.data)
            self.disc_v = torch.zeros_like(self.disc_flat.data)
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

    def step(self, raw_images: torch.Tensor, eps: Optional[torch.Tensor] = None,
             epoch: int = 0) -> Dict[str, torch.Tensor]:
        """``raw_images``: the batch in [0, 1], NCHW fp32 on the device; ``eps``: the posterior noise (None: drawn
        on the device; a VQVAE takes none); ``epoch``: the reference's epoch number, read by the discriminator gate
        only.  Returns VAECriterion's totals as device scalars (``loss`` detached).

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
        active = self.disc is not None and self.criterion.disc_is_active(self.disc, epoch, self.global_step)
        self.flat.grad.zero_()
        if active:
            self.disc_flat.grad.zero_()
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
        out["loss"].backward()
        out["loss"] = out["loss"].detach()
        if active:
            real_pred = self.disc(raw_images.detach())
            fake_pred_detached = self.disc.forward_image(rec.detach(), self.image_map)
            d_gan = self.criterion.discriminator_loss(real_pred, fake_pred_detached)
            d_gan.backward()
            out["d_gan"] = d_gan.detach()
        self.global_step += 1
        from ...runtime import ops
        n = self.n_trained
        ops.adamw(self.flat.data[:n], self.flat.grad[:n], self.m[:n], self.v[:n], self.lr, self.betas[0],
                  self.betas[1], self.eps, self.weight_decay, self.global_step)
        self.eng.invalidate_weights()
        if active:
            self.disc_step += 1
            ops.adamw(self.disc_flat.data, self.disc_flat.grad, self.disc_m, self.disc_v, self.disc_lr,
                      self.betas[0], self.betas[1], self.eps, self.disc_weight_decay, self.disc_step)
            self.disc_eng.invalidate_weights()
        return out

    def disc_state_dict(self) -> Dict[str, Any]:
        """The discriminator optimizer's state in ``torch.optim.AdamW.state_dict()`` form (state keyed by the index
        in ``discriminator.parameters()``)."""
        if self.disc is None:
            raise RuntimeError("VAETrainStep.disc_state_dict: no discriminator")
        params = list(self.disc.parameters())
        state = {}
        if self.disc_step > 0:
            for i, p in enumerate(params):
                off, n = self.disc_flat.offsets[id(p)]
                state[i] = {"step": torch.tensor(float(self.disc_step)),
                            "exp_avg": self.disc_m[off:off + n].view_as(p).detach().cpu().clone(),
                            "exp_avg_sq": self.disc_v[off:off + n].view_as(p).detach().cpu().clone()}
        group = {"lr": self.disc_lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.disc_weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": True, "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group]}

    def load_disc_state_dict(self, sd: Dict[str, Any]) -> None:
        """Inverse of ``disc_state_dict`` (also takes a torch AdamW state of the same discriminator)."""
        if self.disc is None:
            raise RuntimeError("VAETrainStep.load_disc_state_dict: no discriminator")
        st = sd.get("state", {})
        steps = 0
        with torch.no_grad():
            self.disc_m.zero_()
            self.disc_v.zero_()
            for i, p in enumerate(self.disc.parameters()):
                e = st.get(i) if i in st else st.get(str(i))
                if not e:
                    continue
                off, n = self.disc_flat.offsets[id(p)]
                self.disc_m[off:off + n].copy_(torch.as_tensor(e["exp_avg"]).reshape(-1))
                self.disc_v[off:off + n].copy_(torch.as_tensor(e["exp_avg_sq"]).reshape(-1))
                steps = max(steps, int(float(torch.as_tensor(e["step"]))))
        self.disc_step = steps
        groups = sd.get("param_groups") or []
        if groups:
            self.disc_lr = float(groups[0].get("lr", self.disc_lr))
            self.disc_weight_decay = float(groups[0].get("weight_decay", self.disc_weight_decay))

    def state_dict(self) -> Dict[str, Any]:
        """The optimizer state in ``torch.optim.AdamW.state_dict()`` form (state keyed by the index in
        ``model.parameters()``) plus ``global_step``."""
        params = list(self.model.parameters())
        state = {}
        if self.global_step > 0:
            for i, p in enumerate(params):
                off, n = self.flat.offsets[id(p)]
                state[i] = {"step": torch.tensor(float(self.global_step)),
                            "exp_avg": self.m[off:off + n].view_as(p).detach().cpu().clone(),
                            "exp_avg_sq": self.v[off:off + n].view_as(p).detach().cpu().clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "decoupled_weight_decay": True, "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group], "global_step": self.global_step}

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Inverse of ``state_dict`` (also takes a torch AdamW state of the same model)."""
        params = list(self.model.parameters())
        st = sd.get("state", {})
        steps = 0
        with torch.no_grad():
            self.m.zero_()
            self.v.zero_()
            for i, p in enumerate(params):
                e = st.get(i) if i in st else st.get(str(i))
                if not e:
                    continue
                off, n = self.flat.offsets[id(p)]
                self.m[off:off + n].copy_(torch.as_tensor(e["exp_avg"]).reshape(-1))
                self.v[off:off + n].copy_(torch.as_tensor(e["exp_avg_sq"]).reshape(-1))
                steps = max(steps, int(float(torch.as_tensor(e["step"]))))
        self.global_step = int(sd.get("global_step", steps))
        groups = sd.get("param_groups") or []
        if groups:
            g = groups[0]
            self.lr = float(g.get("lr", self.lr))
            self.weight_decay = float(g.get("weight_decay", self.weight_decay))
            self.betas = tuple(float(b) for b in g.get("betas", self.betas))
            self.eps = float(g.get("eps", self.eps))


def train(dataset, json_path, val_dataset=None, resume=None) -> None:
    raise NotImplementedError("The VAE trainer loop is not built: the datasets, checkpoints and sample images "
                              "around the step are still missing "
                              "(DESIGN.md section 7).  One AutoencoderKL or VQVAE optimizer step, with or without a "
                              "discriminator and the perceptual term, is VAETrainStep; the "
                              "criterion it calls is VAECriterion; the quantizer half is "
                              "VectorQuantizer*.quantize_train.")
