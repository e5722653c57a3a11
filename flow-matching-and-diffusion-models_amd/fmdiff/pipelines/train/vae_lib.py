"""VAE trainer pieces (reference ``src/pipelines/train/vae_lib.py``): the scheduler factory, the discriminator
gate and the training criterion as one object over the HIP loss kernels (``fmdiff.nn.losses.vae``,
``csrc/vae_loss.hip``).  The trainer loop itself is not built: it needs the encoder / decoder backward, the
discriminator and the perceptual loss."""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from ...nn.losses.vae import discriminator_hinge_loss, generator_hinge_loss, recon_loss

__all__ = ["VAECriterion", "train"]

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

        total = recon + kl_scale(step) * kl.mean() + effective_codebook_weight * vq_loss + gan_weight * g_gan

    ``recon`` is ``recon_loss(rec, target, recon_type)``; ``kl`` the per-sample KL of ``reparameterize_kl`` /
    ``VAEEngine.kl_forward``; ``vq_loss`` the quantizer's; ``g_gan = generator_hinge_loss(fake_pred)``.  A call
    returns the parts as a dict of device scalars under the reference's ``totals`` keys (absent parts are a device
    zero); ``out["loss"]`` carries the gradient.  Nothing in it synchronises with the host: ``global_step`` is a
    host integer that only selects the host-side ``kl_scale`` factor."""

    def __init__(self, training_cfg: Dict[str, Any], model_cfg: Optional[Dict[str, Any]] = None) -> None:
        model_cfg = model_cfg or {}
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
        if self.perceptual_weight > 0:
            raise NotImplementedError("The VGG perceptual loss (VAE training) is outside the fmdiff hot path; set "
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
                 global_step: int = 0, channels: Optional[int] = None,
                 grad_bf16: Optional[list] = None) -> Dict[str, torch.Tensor]:
        """``rec``: the raw decoder output (channels-first, or with ``channels=C`` the head's channels-last
        output read in place); ``target``: the image in [0, 1], channels-first.  ``fake_pred``: the
        discriminator's logits on the reconstruction when it is active."""
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
        g_gan = zero
        if fake_pred is not None:
            g_gan = generator_hinge_loss(fake_pred)
            total = total + self.gan_weight * g_gan
        return {"loss": total, "recon": recon.detach(), "kl": kl_term.detach(), "perceptual": zero,
                "g_gan": g_gan.detach(), "d_gan": zero, "vq": vq.detach()}

    def discriminator_loss(self, real_pred: torch.Tensor, fake_pred: torch.Tensor) -> torch.Tensor:
        """``d_gan``: the hinge loss of the discriminator on real and (detached) reconstructed images."""
        return discriminator_hinge_loss(real_pred, fake_pred)


def train(dataset, json_path, val_dataset=None, resume=None) -> None:
    raise NotImplementedError("The VAE trainer loop is not built: it needs the encoder / decoder backward, the "
                              "discriminator and the perceptual loss (DESIGN.md section 7).  The criterion it "
                              "would call is VAECriterion; the quantizer half is VectorQuantizer*.quantize_train.")
