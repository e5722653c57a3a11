"""Losses of VAE training (reference ``src/nn/losses/vae.py``): the same names and signatures over the HIP
criterion kernels (``csrc/vae_loss.hip``, ``fmdiff.runtime.ops.elementwise_loss``).

Every function is one ``torch.autograd.Function`` per term: forward is one loss-and-reduce launch (fp64 sums in a
fixed order, the same bits on every run), backward is one launch that recomputes the unit gradient from the saved
input and multiplies it by the upstream gradient read from device memory.  Nothing synchronises with the host, so
a whole criterion step can be captured in a graph.  Inputs are ROCm device tensors: there is no CPU path.  The
gradient goes to the first argument (logits / reconstruction / latents / predictions); targets get none.

``recon_loss`` fuses ``raw_output_to_image`` with the reconstruction loss of the trainer
(``src/pipelines/train/vae_lib.py:228-239``) and also reads the decoder head's channels-last fp32 output in place.

``PerceptualLoss`` refuses and names ``fmdiff.nn.losses.VGGPerceptualLoss`` (``perceptual.py``), which is built;
``PatchDiscriminator`` refuses and names ``fmdiff.nn.modules.vae.discriminators.PatchGANDiscriminatorND``, which is
(DESIGN.md section 7)."""
from __future__ import annotations

from typing import Iterable, Optional, Tuple

import torch
import torch.nn as nn

__all__ = ["PerceptualLoss", "PatchDiscriminator", "discriminator_hinge_loss", "generator_hinge_loss",
           "vq_regularizer", "focal_loss", "bce_focal_loss", "recon_loss"]


class _ElementwiseLoss(torch.autograd.Function):
    """loss (or the per-element term) of ``x``; ``channels``: x is the head's channels-last output.  ``bf16``
    receives the bf16 copy of the gradient in backward (a one-element list the caller keeps), the operand of
    ``ops.head_dgrad``."""

    @staticmethod
    def forward(ctx, x, target, term, reduction, alpha, channels, bf16):
        from ...runtime import ops
        xd = x.detach()
        out = ops.elementwise_loss(term, xd, target, reduction=reduction, alpha=alpha, channels=channels)
        ctx.save_for_backward(xd, target)
        ctx.cfg = (term, reduction, alpha, channels, bf16)
        return out.elem if reduction == "none" else out.loss

    @staticmethod
    def backward(ctx, g):
        from ...runtime import ops
        x, target = ctx.saved_tensors
        term, reduction, alpha, channels, bf16 = ctx.cfg
        g = g.float().contiguous()
        out = ops.elementwise_loss(term, x, target, reduction=reduction, alpha=alpha, channels=channels, g=g,
                                   loss=False, grad=True, grad_bf16=bf16 is not None)
        if bf16 is not None:
            bf16[:] = [out.dx_bf16]
        return out.dx, None, None, None, None, None, None


def _apply(term, x, target=None, reduction="mean", alpha=0.25, channels=None, bf16=None):
    from ...runtime import ops
    ops._need_cuda(x, term)
    if target is not None:
        ops._need_cuda(target, term)
        target = target.detach()
    return _ElementwiseLoss.apply(x, target, term, reduction, float(alpha), channels, bf16)


def _gamma2(gamma: float, what: str) -> None:
    if float(gamma) != 2.0:
        raise NotImplementedError(f"{what}: the HIP focal term is built for gamma = 2.0 only (got {gamma})")


class PerceptualLoss(nn.Module):
    def __init__(self, resize: bool = False, layers: Tuple[int, ...] = (3, 8, 15, 22),
                 layer_weights: Iterable[float] = (1.0, 1.0, 1.0, 1.0)) -> None:
        super().__init__()
        raise NotImplementedError("the VGG perceptual loss is fmdiff.nn.losses.VGGPerceptualLoss (the topology with "
                                  "user-supplied weights: no torchvision, no download); this name is not routed to it")


class PatchDiscriminator(nn.Module):
    def __init__(self, in_channels: int = 1, base_channels: int = 64, spatial_dims: int = 2) -> None:
        super().__init__()
        raise NotImplementedError("the PatchGAN discriminator is fmdiff.nn.modules.vae.discriminators."
                                  "PatchGANDiscriminatorND; this name is not routed to it yet")


def discriminator_hinge_loss(real_pred: torch.Tensor, fake_pred: torch.Tensor) -> torch.Tensor:
    """``mean(relu(1 - real_pred)) + mean(relu(1 + fake_pred))``; the gradient is 0 at the kinks."""
    return _apply("hinge_real", real_pred) + _apply("hinge_fake", fake_pred)


def generator_hinge_loss(fake_pred: torch.Tensor) -> torch.Tensor:
    """``-mean(fake_pred)``."""
    return _apply("neg", fake_pred)


def vq_regularizer(latents: torch.Tensor) -> torch.Tensor:
    """The reference's ``mean(mean_c^2) + mean((x - mean_c)^2)`` with ``mean_c`` the per-channel mean over batch
    and space.  The two terms add up to ``mean(x^2)`` identically: with n_c elements per channel,
    ``sum_c sum_i (x_ci - m_c)^2 = sum_c (sum_i x_ci^2 - n_c m_c^2)`` and every channel has the same n_c, so the
    per-channel mean terms cancel.  It is therefore built as the ``square`` term (one pass, no per-channel
    statistics); ``tests/test_vae_loss_bounds.py`` proves the identity in fp64."""
    return _apply("square", latents)


def focal_loss(logits: torch.Tensor, targets: torch.Tensor, alpha: float = 0.25, gamma: float = 2.0,
               reduction: str = "mean") -> torch.Tensor:
    """Binary focal loss on logits, ``alpha_t (1 - p_t)^2 ce``; targets may be soft."""
    _gamma2(gamma, "focal_loss")
    return _apply("focal", logits, targets, _reduction(reduction), alpha)


def bce_focal_loss(logits: torch.Tensor, targets: torch.Tensor, alpha: float = 0.25, gamma: float = 2.0,
                   reduction: str = "mean") -> torch.Tensor:
    """BCE + focal on logits in one pass (the reference reduces the two and adds the results)."""
    _gamma2(gamma, "bce_focal_loss")
    return _apply("bce_focal", logits, targets, _reduction(reduction), alpha)


def _reduction(reduction: str) -> str:
    # the reference returns the unreduced tensor for anything but "mean" and "sum"
    return reduction if reduction in ("mean", "sum") else "none"


_RECON_TERMS = {"l1": "l1", "mse": "mse", "bce": "bce", "focal": "bce_focal", "bce_focal": "bce_focal"}


def recon_loss(rec: torch.Tensor, target: torch.Tensor, recon_type: str = "l1", *, channels: Optional[int] = None,
               grad_bf16: Optional[list] = None) -> torch.Tensor:
    """The trainer's reconstruction loss of the raw decoder output ``rec`` against the image ``target`` in
    [0, 1]: ``l1`` / ``mse`` of ``(clamp(rec, -1, 1) + 1) / 2``, ``bce`` on the logits, and ``focal`` and
    ``bce_focal`` both ``bce_focal_loss(alpha=0.25, gamma=2)``, as the trainer maps them.  ``channels=C``: ``rec`` is
    the decoder head's channels-last fp32 output ``[N, *spatial, >= C]`` read in place (``target`` stays
    channels-first); ``grad_bf16``: a list that receives the bf16 copy of the gradient in backward."""
    if recon_type not in _RECON_TERMS:
        raise ValueError(f"Unsupported recon_type '{recon_type}'.")
    return _apply(_RECON_TERMS[recon_type], rec, target, "mean", 0.25, channels, grad_bf16)
