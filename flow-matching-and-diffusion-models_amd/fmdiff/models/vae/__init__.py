"""VAE models (reference ``src/models/vae/__init__.py``): ``AutoencoderKL`` and ``VQVAE``, forward / inference
on the HIP engine.  Their training (losses, discriminators, the EMA codebook update) is out of scope."""
from .base import BaseVAE
from .kl import LATENT_SCALE, AutoencoderKL
from .vq import VQVAE

__all__ = ["BaseVAE", "AutoencoderKL", "VQVAE", "LATENT_SCALE"]
