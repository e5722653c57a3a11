"""Vector-quantizer codebooks (reference ``src/nn/modules/vae/codebook.py:12-137``): same constructors,
attributes, state_dict keys and return tuple.  These are parameter holders: ``forward`` hands the latent and
the fp32 codebook to the HIP quantizer (``fmdiff.runtime.ops.vq_quantize``, ``csrc/vq.hip``), which finds the
nearest code on MFMA without the reference's M x K distance and one-hot matrices and returns
``(quantized, vq_loss, perplexity, codes)`` as device tensors without a host synchronisation.

Forward only: the outputs carry no gradient, and the EMA codebook update of a training-mode
``VectorQuantizerEMA`` belongs to VAE training."""
from __future__ import annotations

import torch
import torch.nn as nn

__all__ = ["VectorQuantizer", "VectorQuantizerEMA"]


class _VectorQuantizerBase(nn.Module):
    classic = False   # vq_loss = (1 + beta) mse (codebook + commitment terms) instead of beta mse

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25) -> None:
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.commitment_cost = commitment_cost

    def _stats_eps(self) -> float:
        return 1e-5

    def _check_forward_only(self) -> None:
        pass

    @torch.no_grad()
    def quantize_nhwc(self, z_nhwc: torch.Tensor, Cpad=None):
        """The engine's entry: ``z_nhwc`` fp32 channels-last ``[N, *spatial, >= embedding_dim]``."""
        from ....runtime import ops
        self._check_forward_only()
        return ops.vq_quantize(z_nhwc, self.embedding_dim, self.embedding, self.commitment_cost, self.classic,
                               eps=self._stats_eps(), Cpad=Cpad)

    def forward(self, z: torch.Tensor):
        from ....runtime import ops
        self._check_forward_only()
        ops._need_cuda(z, type(self).__name__)
        if z.dim() < 2 or z.shape[1] != self.embedding_dim:
            raise ValueError(f"{type(self).__name__}: expected [N, {self.embedding_dim}, *spatial], got "
                             f"{tuple(z.shape)}")
        out = self.quantize_nhwc(z.detach().float().movedim(1, -1).contiguous())
        return out.zq, out.vq_loss, out.perplexity, out.codes


class VectorQuantizer(_VectorQuantizerBase):
    """Original VQ-VAE quantizer (the codebook is a parameter)."""
    classic = True

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25) -> None:
        super().__init__(num_embeddings, embedding_dim, commitment_cost)
        self.embedding = nn.Parameter(torch.randn(num_embeddings, embedding_dim))


class VectorQuantizerEMA(_VectorQuantizerBase):
    """Codebook kept by exponential moving averages (buffers); inference here, the update is training."""

    def __init__(self, num_embeddings: int, embedding_dim: int, commitment_cost: float = 0.25, decay: float = 0.99,
                 eps: float = 1e-5) -> None:
        super().__init__(num_embeddings, embedding_dim, commitment_cost)
        self.decay = decay
        self.eps = eps
        embedding = torch.randn(num_embeddings, embedding_dim)
        self.register_buffer("embedding", embedding)
        self.register_buffer("ema_cluster_size", torch.zeros(num_embeddings))
        self.register_buffer("ema_w", embedding.clone())

    def _stats_eps(self) -> float:
        return self.eps

    def _check_forward_only(self) -> None:
        if self.training and self.decay > 0.0:
            raise NotImplementedError("VectorQuantizerEMA: the EMA codebook update is VAE training, outside the "
                                      "fmdiff hot path; call .eval() (or set decay=0) for the forward pass")
