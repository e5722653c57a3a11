"""Generate the discriminator golden fixture from the reference itself.

Run on the build machine only (the reference never travels to the GPU machine), with the reference checkout's root in
``FMDIFF_REFERENCE``:

    FMDIFF_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_disc_golden.py

Runs the reference's own ``nn.modules.vae.discriminators.MagvitDiscriminatorND`` and
``nn.losses.vae.PatchDiscriminator`` (pure PyTorch, CPU, fp32) with ``base_channels`` 8, so that the file stays
below 1 MiB (0.89 MiB: the two state_dicts and their gradients are 0.17 MiB each).  For each of ``CASES``:

* ``sd.<key>``: the seeded state_dict (torch's own initialisation under ``torch.manual_seed``, then BatchNorm weights,
  biases and running statistics redrawn away from their 1 / 0 defaults, so that a swapped gamma / beta or a missed
  running-statistics update shows);
* ``x``: one seeded input, ``g``: a seeded cotangent of the logits;
* ``train.logits``: the training-mode logits; ``train.buf.<key>``: every buffer after that pass
  (``num_batches_tracked`` included); ``train.dx`` and ``train.grad.<key>``: the gradients of ``(logits * g).sum()``
  to the input and to every parameter;
* ``eval.logits``: an eval-mode pass from the seeded state_dict (buffers before the training pass).

Tensors only; load with ``weights_only=True``.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.environ["FMDIFF_REFERENCE"], "src"))

from nn.losses.vae import PatchDiscriminator  # noqa: E402  (reference)
from nn.modules.vae.discriminators import MagvitDiscriminatorND  # noqa: E402  (reference)

CASES = {"magvit": (MagvitDiscriminatorND, 1, (3, 1, 48, 64), 11), "patchgan": (PatchDiscriminator, 3, (3, 3, 32, 48), 12)}
BASE = 8


def seeded(cls, in_channels, seed):
    torch.manual_seed(seed)
    m = cls(in_channels=in_channels, base_channels=BASE, spatial_dims=2)
    g = torch.Generator().manual_seed(seed + 100)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            with torch.no_grad():
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.3)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
    return m


def main():
    out = {}
    for name, (cls, cin, shape, seed) in CASES.items():
        m = seeded(cls, cin, seed)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        gen = torch.Generator().manual_seed(seed + 200)
        x = torch.randn(shape, generator=gen)
        m.eval()
        with torch.no_grad():
            ev = m(x).clone()
        m.load_state_dict(sd)
        m.train()
        xr = x.clone().requires_grad_()
        logits = m(xr)
        g = torch.randn(logits.shape, generator=gen)
        (logits * g).sum().backward()
        for k, v in sd.items():
            out[f"{name}.sd.{k}"] = v
        out[f"{name}.x"], out[f"{name}.g"] = x, g
        out[f"{name}.train.logits"] = logits.detach().clone()
        out[f"{name}.train.dx"] = xr.grad.clone()
        for k, v in m.named_buffers():
            out[f"{name}.train.buf.{k}"] = v.detach().clone()
        for k, p in m.named_parameters():
            out[f"{name}.train.grad.{k}"] = p.grad.clone()
        out[f"{name}.eval.logits"] = ev
    path = os.path.join(HERE, "disc_golden.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes,", len(out), "tensors")


if __name__ == "__main__":
    main()
