"""Generate the VAE-criterion golden fixture from the reference itself.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vae_loss_golden.py

Runs the reference's ``nn.losses.vae`` functions, the trainer's reconstruction losses
(``pipelines/train/vae_lib.py:228-239`` over ``BaseAutoencoder.raw_output_to_image``) and
``nn.modules.vae.reparameterizer.DiagonalGaussian`` (pure PyTorch, CPU, fp32; torchvision is not needed) and
writes ``vae_loss_golden.pt``, tensors only (load with ``weights_only=True``).

Shapes: N = 2, C in {1, 3}, spatial (5, 7) and (3, 5, 7), tags ``c{C}_{2d|3d}``; moments (2, 8, 5, 7).  Inputs are
seeded (``vae_loss_bounds.gen``) with planted values (``vae_loss_bounds.plant_*``): ``rec`` at exactly +-1, just
inside and just outside, and where img == target; logits at +-100, +-5 and 0 against targets 0, 1 and soft;
logvar at -31, -30, 0, 20 and 21; discriminator logits at exactly +-1.

Recorded per tag: ``rec``, ``target``, ``logits``, ``soft`` (targets in [0, 1]); for every recon_type the trainer's
loss (``recon.<type>``) and the gradient of ``0.7 * loss`` to the raw decoder output (``recon.<type>.grad``; l1 / mse
on ``rec`` against ``target``, the logit losses on ``logits`` against ``soft``); for ``focal_loss`` and
``bce_focal_loss`` and each reduction the value (``<fn>.<reduction>``) and the gradient of ``0.7 * loss`` (summed for
``none``) to the logits.  Once: both hinge losses and ``vq_regularizer`` with the gradients of ``0.7 * loss`` to
their inputs, and ``DiagonalGaussian(moments)``: ``sample()`` with the recorded ``eps`` (``randn_like`` patched),
``kl()``, and the gradient of ``(z * g_z).sum() + 0.7 * kl.mean()`` to the moments.  Targets get no gradient.
"""
from __future__ import annotations

import os
import sys
from unittest import mock

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join("/root/reference", "src"))
sys.path.insert(0, os.path.dirname(HERE))

from models.autoencoder.base import BaseAutoencoder  # noqa: E402  (reference)
from nn.losses.vae import (bce_focal_loss, discriminator_hinge_loss, focal_loss,  # noqa: E402  (reference)
                           generator_hinge_loss, vq_regularizer)
from nn.modules.vae.reparameterizer import DiagonalGaussian  # noqa: E402  (reference)

import vae_loss_bounds as lb  # noqa: E402

G = 0.7
SHAPES = {"c1_2d": (2, 1, 5, 7), "c3_2d": (2, 3, 5, 7), "c1_3d": (2, 1, 3, 5, 7), "c3_3d": (2, 3, 3, 5, 7)}
RECON_TYPES = ("l1", "mse", "bce", "focal", "bce_focal")


def inputs(tag, shape):
    g = lb.gen(f"vae_loss/{tag}")
    rec, target = lb.plant_rec(torch.randn(shape, generator=g) * 1.2, torch.rand(shape, generator=g))
    logits, soft = lb.plant_logits(torch.randn(shape, generator=g) * 3.0, torch.rand(shape, generator=g))
    hard = torch.rand(shape, generator=g) < 0.5            # half of the random targets are exactly 0 or 1
    pick = torch.rand(shape, generator=g) < 0.5
    pick.view(-1)[:15] = False                             # the planted pairs stay
    soft = torch.where(pick, hard.float(), soft)
    return rec, target, logits, soft


def trainer_recon(rec, raw_chunk, recon_type):
    """vae_lib.py:228-239 with the reference's own functions."""
    rec_img = BaseAutoencoder.raw_output_to_image(_Range(), rec, recon_type=recon_type)
    if recon_type == "l1":
        return F.l1_loss(rec_img, raw_chunk)
    if recon_type == "mse":
        return F.mse_loss(rec_img, raw_chunk)
    if recon_type == "bce":
        return F.binary_cross_entropy_with_logits(rec, raw_chunk)
    return bce_focal_loss(rec, raw_chunk, alpha=0.25, gamma=2.0, reduction="mean")


class _Range:
    model_to_image_range = BaseAutoencoder.model_to_image_range


def with_grad(fn, *xs):
    leaves = [x.clone().requires_grad_() for x in xs]
    loss = fn(*leaves)
    (G * loss).sum().backward()
    return loss.detach().clone(), [leaf.grad.clone() for leaf in leaves]


def main():
    torch.set_num_threads(8)
    out = {}
    for tag, shape in SHAPES.items():
        rec, target, logits, soft = inputs(tag, shape)
        out.update({f"{tag}.rec": rec, f"{tag}.target": target, f"{tag}.logits": logits, f"{tag}.soft": soft})
        for rt in RECON_TYPES:
            x, t = (rec, target) if rt in ("l1", "mse") else (logits, soft)
            v, (gx,) = with_grad(lambda a: trainer_recon(a, t, rt), x)
            out[f"{tag}.recon.{rt}"], out[f"{tag}.recon.{rt}.grad"] = v, gx
        for name, fn in (("focal_loss", focal_loss), ("bce_focal_loss", bce_focal_loss)):
            for red in ("mean", "sum", "none"):
                v, (gx,) = with_grad(lambda a: fn(a, soft, alpha=0.25, gamma=2.0, reduction=red), logits)
                out[f"{tag}.{name}.{red}"], out[f"{tag}.{name}.{red}.grad"] = v, gx
    g = lb.gen("vae_loss/once")
    real, fake = lb.plant_disc(torch.randn(2, 1, 3, 4, generator=g) * 1.5), lb.plant_disc(
        torch.randn(2, 1, 3, 4, generator=g) * 1.5)
    v, (gr, gf) = with_grad(discriminator_hinge_loss, real, fake)
    out.update({"disc.real": real, "disc.fake": fake, "disc.d_loss": v, "disc.d_loss.grad_real": gr,
                "disc.d_loss.grad_fake": gf})
    v, (gf,) = with_grad(generator_hinge_loss, fake)
    out.update({"disc.g_loss": v, "disc.g_loss.grad": gf})
    lat = torch.randn(2, 4, 5, 7, generator=g) * 1.3 + 0.4
    v, (gl,) = with_grad(vq_regularizer, lat)
    out.update({"vqreg.latents": lat, "vqreg.loss": v, "vqreg.grad": gl})

    moments = lb.plant_logvar(torch.randn(2, 8, 5, 7, generator=g) * 2.0)
    eps = torch.randn(2, 4, 5, 7, generator=g)
    g_z = torch.randn(2, 4, 5, 7, generator=g)
    m = moments.clone().requires_grad_()
    with mock.patch.object(torch, "randn_like", lambda t, **kw: eps):
        post = DiagonalGaussian(m)
        z = post.sample()
    kl = post.kl()
    ((z * g_z).sum() + G * kl.mean()).backward()
    out.update({"post.moments": moments, "post.eps": eps, "post.g_z": g_z, "post.z": z.detach().clone(),
                "post.kl": kl.detach().clone(), "post.grad": m.grad.clone(),
                "post.mode": DiagonalGaussian(moments).mode().clone()})
    out["hyper"] = torch.tensor([G, 0.25, 2.0], dtype=torch.float64)
    path = os.path.join(HERE, "vae_loss_golden.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "tensors")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
