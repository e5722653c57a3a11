"""``VQVAE`` (reference ``src/models/vae/vq.py:23-183``): same constructor, attributes and state_dict keys.
``encode`` runs the encoder with ``quant_conv`` folded into its output conv, ``decode`` runs
``post_quant_conv`` and the decoder, and ``forward`` chains encoder -> HIP quantizer (``csrc/vq.hip``) ->
decoder on the fused engine (``fmdiff.runtime.vae_engine``) with the quantized latent handed over as the NHWC
bf16 operand the decoder reads, so there is no channels-first round trip.  ``forward_train`` is the same chain under
a tape, connected to the parameters by autograd (training; ``forward`` itself carries no gradient).

``quantizer_type``: ``"classic"`` / ``"vq"`` (codebook parameter) or ``"ema"`` (codebook buffers);
``make_discriminator`` builds the MAGVIT discriminator for ``discriminator_type == "magvit"``
(``fmdiff.nn.modules.vae.discriminators``)."""
from __future__ import annotations

import os
import warnings
from typing import Optional, Tuple

import torch

from ...nn.modules.vae import Decoder, Encoder
from ...nn.modules.vae.codebook import VectorQuantizer, VectorQuantizerEMA
from ...nn.ops.convolution import ConvND
from .base import BaseVAE

LATENT_SCALE: float = 0.18215


class VQVAE(BaseVAE):
    def __init__(self, in_channels: int = 3, out_channels: int = 3, resolution: int = 256, base_ch: int = 128,
                 ch_mult: Tuple[int, ...] = (1, 2, 4, 4), down_channels: Tuple[int, ...] | None = None,
                 num_res_blocks: int = 2, attn_resolutions: Tuple[int, ...] = (), z_channels: int = 4,
                 embed_dim: int = 4, dropout: float = 0.0, use_attention: bool = True, attn_heads: int = 4,
                 attn_dim_head: int = 64, spatial_dims: int = 2, emb_channels: Optional[int] = None,
                 use_scale_shift_norm: bool = False, ckpt_path: Optional[str] = None, codebook_size: int = 1024,
                 vq_beta: float = 0.25, vq_ema_decay: float = 0.99, vq_ema_eps: float = 1e-5,
                 quantizer_type: str = "ema", discriminator_type: str = "patchgan", block_factory=None) -> None:
        super().__init__()
        self.spatial_dims = spatial_dims
        self.quantizer_type = str(quantizer_type).lower()
        self.discriminator_type = str(discriminator_type).lower() if discriminator_type is not None else "patchgan"
        common = dict(base_ch=base_ch, ch_mult=ch_mult, down_channels=down_channels, num_res_blocks=num_res_blocks,
                      attn_resolutions=attn_resolutions, resolution=resolution, z_channels=z_channels,
                      dropout=dropout, use_attention=use_attention, attn_heads=attn_heads,
                      attn_dim_head=attn_dim_head, spatial_dims=spatial_dims, emb_channels=emb_channels,
                      use_scale_shift_norm=use_scale_shift_norm, block_factory=block_factory)
        self.encoder = Encoder(in_channels=in_channels, double_z=False, **common)
        self.decoder = Decoder(out_ch=out_channels, tanh_out=False, **common)
        self.quant_conv = ConvND(spatial_dims, z_channels, embed_dim, 1, padding=0)
        self.post_quant_conv = ConvND(spatial_dims, embed_dim, z_channels, 1, padding=0)
        self.embed_dim = embed_dim
        self.codebook = self._build_quantizer(codebook_size=codebook_size, embed_dim=embed_dim, vq_beta=vq_beta,
                                              vq_ema_decay=vq_ema_decay, vq_ema_eps=vq_ema_eps)
        if ckpt_path:
            if not os.path.exists(ckpt_path):
                raise FileNotFoundError(f"Checkpoint not found: {ckpt_path}")
            self.load_state_dict(torch.load(ckpt_path, map_location="cpu", weights_only=True))
        else:
            warnings.warn("[VQVAE] No checkpoint provided. Random initialization.")

    def _build_quantizer(self, *, codebook_size: int, embed_dim: int, vq_beta: float, vq_ema_decay: float,
                         vq_ema_eps: float):
        if self.quantizer_type in {"classic", "vq"}:
            return VectorQuantizer(num_embeddings=codebook_size, embedding_dim=embed_dim, commitment_cost=vq_beta)
        if self.quantizer_type == "ema":
            return VectorQuantizerEMA(num_embeddings=codebook_size, embedding_dim=embed_dim,
                                      commitment_cost=vq_beta, decay=vq_ema_decay, eps=vq_ema_eps)
        raise ValueError(f"Unknown quantizer_type '{self.quantizer_type}'. Expected 'classic' or 'ema'.")

    def _engine(self):
        from ...runtime.vae_engine import get_vae_engine
        if self.spatial_dims != 2:
            raise NotImplementedError("fmdiff VAE engine: spatial_dims=2")
        return get_vae_engine(self)

    def make_discriminator(self):
        """The reference's ``VQVAE.make_discriminator`` (``src/models/vae/vq.py``) for the MAGVIT discriminator."""
        if self.discriminator_type == "magvit":
            from ...nn.modules.vae.discriminators import MagvitDiscriminatorND
            return MagvitDiscriminatorND(in_channels=self.decoder.conv_out.conv.out_channels,
                                         spatial_dims=self.spatial_dims)
        return super().make_discriminator()

    def encode(self, x: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        quant_in = self._engine().encode_moments(x)
        if normalize:
            return quant_in * LATENT_SCALE
        return quant_in

    def decode(self, z: torch.Tensor, denorm: bool = False) -> torch.Tensor:
        if denorm:
            z = z / LATENT_SCALE
        return self._engine().decode(z)

    def forward(self, x: torch.Tensor):
        rec, q = self._engine().vq_forward(x)
        return rec, {"vq_loss": q.vq_loss, "perplexity": q.perplexity, "codes": q.codes}

    def forward_train(self, x: torch.Tensor):
        """``forward`` for training: the same tuple, with ``rec`` and ``vq_loss`` connected to the parameters by
        autograd (``fmdiff.runtime.vae_engine.vqvae_forward_train``; perplexity and codes carry no gradient).  A
        training-mode EMA codebook is updated by this call, as the reference's forward does; the classic codebook
        parameter gets no gradient, as in the reference."""
        from ...runtime.vae_engine import vqvae_forward_train
        self._engine()
        rec, vq_loss, perplexity, codes = vqvae_forward_train(self, x)
        return rec, {"vq_loss": vq_loss, "perplexity": perplexity, "codes": codes}
