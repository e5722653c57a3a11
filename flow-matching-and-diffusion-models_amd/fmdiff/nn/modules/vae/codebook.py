"""Vector-quantizer codebooks (reference ``src/nn/modules/vae/codebook.py:12-137``): same constructors,
attributes, state_dict keys and return tuple.  These are parameter holders: ``forward`` hands the latent and
the fp32 codebook to the HIP quantizer (``fmdiff.runtime.ops.vq_quantize``, ``csrc/vq.hip``), which finds the
nearest code on MFMA without the reference's M x K distance and one-hot matrices and returns
``(quantized, vq_loss, perplexity, codes)`` as device tensors without a host synchronisation.

``forward`` is inference: its outputs carry no gradient and a training-mode ``VectorQuantizerEMA`` refuses it.
Training goes through ``quantize_train`` (``quantize_train_nhwc`` for the engine): the same quantisation, with
``z_q`` and ``vq_loss`` connected to ``z`` by one ``torch.autograd.Function`` whose backward is
``ops.vq_backward`` (``dz = g_zq + g_loss c 2/(MD) (z - q)``, c = beta for the EMA quantizer and beta - 1 for the
classic one, whose codebook gets no gradient, as in the reference), and, on a training-mode
``VectorQuantizerEMA`` with ``decay > 0``, the in-place EMA update of the three buffers after quantising
(``ops.vq_ema_update``, ``csrc/vq_train.hip``: a deterministic per-code segmented sum instead of the reference's
one-hot product).  ``codebook_grad=True`` on the classic quantizer adds the VQ-VAE paper's codebook gradient, a
stated deviation from the reference."""
from __future__ import annotations

import torch
import torch.nn as nn

__all__ = ["VectorQuantizer", "VectorQuantizerEMA"]


def _quantize_and_update(mod, zd, e, update, Cpad):
    """The training-mode quantisation of the detached rows ``zd`` against ``e`` (the codebook object itself: the
    plane cache is keyed on it) and, with ``update``, the EMA update.  Returns ``(ops.VQOut, saved)``: ``saved`` is
    what the latent gradient reads, ``(z - q,)`` when the codebook has been rewritten (all the backward reads of
    it), else ``(z, codes, codebook, hist)``.  One body for ``_QuantizeTrain`` and the engine's VQVAE walk."""
    from ....runtime import ops
    D = mod.embedding_dim
    out = ops.vq_quantize(zd, D, e, mod.commitment_cost, mod.classic, eps=mod._stats_eps(), Cpad=Cpad)
    if update:
        saved = (ops.vq_residual(zd, D, out.codes, e),)
        ops.vq_ema_update(zd, D, out.codes, out.hist, e, mod.ema_cluster_size, mod.ema_w, mod.decay, mod.eps)
    else:
        saved = (zd, out.codes, e, out.hist)
    return out, saved


class _QuantizeTrain(torch.autograd.Function):
    """(z_q channels-first, vq_loss) of channels-last rows ``z_nhwc``; ``embedding`` is an input only for the
    opt-in codebook gradient.  What backward needs is saved before ``update`` overwrites the codebook."""

    @staticmethod
    def forward(ctx, z_nhwc, embedding, mod, update, codebook_grad, Cpad):
        D = mod.embedding_dim
        out, saved = _quantize_and_update(mod, z_nhwc.detach(), embedding, update, Cpad)
        ctx.D, ctx.codebook_grad = D, codebook_grad
        ctx.c = mod._latent_coef()
        ctx.save_for_backward(*saved)
        ctx.update = update
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out.codes, out.perplexity, out.zq_nhwc, out.hist, out.mse)
        return out.zq, out.vq_loss, out.perplexity, out.codes, out.zq_nhwc, out.hist, out.mse

    @staticmethod
    def backward(ctx, g_zq, g_loss, *_):
        from ....runtime import ops
        D = ctx.D
        if g_zq is not None:
            g_zq = g_zq.float().movedim(1, -1).contiguous()
        if g_loss is not None:
            g_loss = g_loss.float().reshape(1)
        dE = None
        if ctx.update:
            (r,) = ctx.saved_tensors
            dz = ops.vq_backward(r, D, None, None, g_zq, g_loss, ctx.c)
        else:
            z, codes, e, hist = ctx.saved_tensors
            dz = ops.vq_backward(z, D, codes, e, g_zq, g_loss, ctx.c)
            if ctx.codebook_grad and ctx.needs_input_grad[1]:
                dE = ops.vq_codebook_grad(z, D, codes, hist, e, g_loss)
        return dz, dE, None, None, None, None


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

    def _updates(self) -> bool:
        return False

    def _latent_coef(self) -> float:
        """``c`` of the latent gradient ``g_loss c 2/(MD) (z - q)``: beta, or beta - 1 for the classic quantizer."""
        return self.commitment_cost - 1.0 if self.classic else self.commitment_cost

    def quantize_train_saved(self, z_nhwc: torch.Tensor, Cpad=None):
        """``quantize_train_nhwc`` without the autograd node, for a caller that runs the backward itself (the
        engine's VQVAE walk, whose latent gradient goes through ``ops.vq_join_bwd``): the same quantisation and,
        in training mode, the same EMA update.  Returns ``(ops.VQOut, saved)`` with ``saved`` as
        ``_quantize_and_update`` describes it; nothing carries a gradient."""
        from ....runtime import ops
        ops._need_cuda(z_nhwc, type(self).__name__)
        with torch.no_grad():
            return _quantize_and_update(self, z_nhwc.detach(), self.embedding, self._updates(), Cpad)

    def quantize_train_nhwc(self, z_nhwc: torch.Tensor, codebook_grad: bool = False, Cpad=None):
        """The engine's training entry: ``z_nhwc`` fp32 channels-last ``[N, *spatial, >= embedding_dim]``.  Returns
        ``ops.VQOut`` whose ``zq`` (channels-first) and ``vq_loss`` carry the gradient to ``z_nhwc`` (padding
        channels get zero); a training-mode EMA quantizer has updated its buffers when this returns."""
        from ....runtime import ops
        ops._need_cuda(z_nhwc, type(self).__name__)
        if codebook_grad and not self.classic:
            raise ValueError("codebook_grad applies to the classic VectorQuantizer: the EMA codebook is a buffer")
        zq, vq_loss, perplexity, codes, zq_nhwc, hist, mse = _QuantizeTrain.apply(
            z_nhwc, self.embedding, self, self._updates(), bool(codebook_grad), Cpad)
        return ops.VQOut(zq, zq_nhwc, vq_loss, perplexity, codes, hist, mse)

    def quantize_train(self, z: torch.Tensor, codebook_grad: bool = False):
        """Training-mode quantisation of ``[N, embedding_dim, *spatial]``: the reference's
        ``(quantized, vq_loss, perplexity, codes)`` with ``quantized`` and ``vq_loss`` differentiable in ``z``;
        ``VectorQuantizerEMA`` in ``.train()`` with ``decay > 0`` then updates its buffers in place."""
        from ....runtime import ops
        ops._need_cuda(z, type(self).__name__)
        if z.dim() < 2 or z.shape[1] != self.embedding_dim:
            raise ValueError(f"{type(self).__name__}: expected [N, {self.embedding_dim}, *spatial], got "
                             f"{tuple(z.shape)}")
        out = self.quantize_train_nhwc(z.float().movedim(1, -1).contiguous(), codebook_grad)
        return out.zq, out.vq_loss, out.perplexity, out.codes

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
    """Codebook kept by exponential moving averages (buffers); ``forward`` is inference, ``quantize_train``
    quantises and then updates the buffers."""

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

    def _updates(self) -> bool:
        return bool(self.training and self.decay > 0.0)

    def _check_forward_only(self) -> None:
        if self.training and self.decay > 0.0:
            raise NotImplementedError("VectorQuantizerEMA: the EMA codebook update is VAE training, outside the "
                                      "fmdiff hot path; call .eval() (or set decay=0) for the forward pass, or "
                                      "quantize_train() for a training step")
