"""``DiagonalGaussian`` (reference ``src/nn/modules/vae/reparameterizer.py:13-62``).

``mode()`` is a channel slice of the moments (no arithmetic); ``sample`` / ``kl`` / ``nll`` are the
reference's small latent-sized elementwise formulas (not on the encode -> denoise -> decode hot path)."""
from __future__ import annotations

import math
from typing import Iterable, Optional

import torch


class DiagonalGaussian:
    def __init__(self, parameters: torch.Tensor, deterministic: bool = False):
        mu, logvar = torch.chunk(parameters, 2, dim=1)
        self.mu = mu
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.deter = deterministic
        self.device = parameters.device
        if deterministic:
            self.std = torch.zeros_like(mu)
            self.var = torch.zeros_like(mu)
        else:
            self.std = torch.exp(0.5 * self.logvar)
            self.var = torch.exp(self.logvar)

    def sample(self) -> torch.Tensor:
        if self.deter:
            return self.mu
        return self.mu + self.std * torch.randn_like(self.mu)

    def mode(self) -> torch.Tensor:
        return self.mu

    def kl(self, other: Optional["DiagonalGaussian"] = None, reduce_dims: Iterable[int] = (1, 2, 3)) -> torch.Tensor:
        if self.deter:
            return torch.tensor([0.0], device=self.device)
        if other is None:
            return 0.5 * torch.sum(self.mu.pow(2) + self.var - 1.0 - self.logvar, dim=reduce_dims)
        return 0.5 * torch.sum((self.mu - other.mu).pow(2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=reduce_dims)

    def nll(self, x: torch.Tensor, reduce_dims: Iterable[int] = (1, 2, 3)) -> torch.Tensor:
        return 0.5 * torch.sum(math.log(2.0 * math.pi) + self.logvar + (x - self.mu).pow(2) / self.var,
                               dim=reduce_dims)


class _ReparameterizeKL(torch.autograd.Function):
    """(z, kl[, staged z]) of the moments in one launch (``csrc/vae_loss.hip``); backward is one launch that
    recomputes from the saved moments and eps."""

    @staticmethod
    def forward(ctx, moments, eps, E, channels_last, Cp):
        from ....runtime import ops
        m = moments.detach()
        if not channels_last:
            m = m.movedim(1, -1).contiguous()
        z, kl, zs = ops.gauss_sample_kl(m, E, eps, Cp=Cp)
        ctx.save_for_backward(m, eps)
        ctx.cfg = (E, channels_last)
        ctx.set_materialize_grads(False)
        if zs is None:
            return z, kl
        ctx.mark_non_differentiable(zs)
        return z, kl, zs

    @staticmethod
    def backward(ctx, g_z, g_kl, *_):
        from ....runtime import ops
        m, eps = ctx.saved_tensors
        E, channels_last = ctx.cfg
        if g_z is not None:
            g_z = g_z.float().contiguous()
        if g_kl is not None:
            g_kl = g_kl.float().contiguous()
        dm, _ = ops.gauss_backward(m, E, eps, g_z, g_kl)
        return (dm if channels_last else dm.movedim(-1, 1)), None, None, None, None


def reparameterize_kl(moments: torch.Tensor, eps: Optional[torch.Tensor] = None, sample: bool = True,
                      generator: Optional[torch.Generator] = None, *, channels_last: bool = False,
                      embed_dim: Optional[int] = None, staged_channels: Optional[int] = None):
    """``DiagonalGaussian(moments).sample()`` (``.mode()`` with ``sample=False``) and ``.kl()`` in one HIP launch:
    returns ``(z [N, E, *spatial], kl_per_sample [N])``, both connected to ``moments`` by one autograd function
    (``d_mu = g_z + g_kl mu``, ``d_logvar = [-30 <= logvar <= 20] (g_z eps std / 2 + g_kl (var - 1) / 2)``).

    ``moments`` is fp32 ``[N, 2E, *spatial]``, or with ``channels_last=True`` the engine's ``[N, *spatial, >= 2E]``
    head output, read in place (``embed_dim`` = E is then required; the gradient comes back in that layout, padding
    channels zero).  ``eps``: the noise, fp32 ``[N, E, *spatial]``; with ``eps=None`` and ``sample=True`` it is
    drawn with ``torch.randn`` on the device (``generator``): the draw is standard normal, but it is NOT the
    random stream of the reference's ``randn_like``, so samples are not comparable number for number.
    ``staged_channels``: also return the decoder's staged operand (bf16 channels-last, that many channels) as a
    third, non-differentiable output.  The KL is computed in the mode path too.  ROCm device tensors only."""
    from ....runtime import ops
    ops._need_cuda(moments, "reparameterize_kl")
    if channels_last:
        if embed_dim is None:
            raise ValueError("reparameterize_kl: channels_last moments need embed_dim")
        E = int(embed_dim)
        shape = (moments.shape[0], E, *moments.shape[1:-1])
    else:
        if moments.dim() < 3 or moments.shape[1] % 2:
            raise ValueError(f"reparameterize_kl: moments [N, 2E, *spatial], got {tuple(moments.shape)}")
        E = moments.shape[1] // 2
        if embed_dim is not None and int(embed_dim) != E:
            raise ValueError(f"reparameterize_kl: embed_dim {embed_dim} against {moments.shape[1]} moment channels")
        shape = (moments.shape[0], E, *moments.shape[2:])
    if not sample:
        eps = None
    elif eps is None:
        eps = torch.randn(shape, device=moments.device, dtype=torch.float32, generator=generator)
    return _ReparameterizeKL.apply(moments, eps, E, bool(channels_last), staged_channels)
