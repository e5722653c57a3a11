"""VAE modules (reference ``src/nn/modules/vae/__init__.py``): encoder, decoder, diagonal Gaussian and the
vector-quantizer codebooks (forward on ``csrc/vq.hip``).

The discriminators of the reference and the EMA codebook update (GAN / VQ-VAE training) are outside the hot
path."""
from .codebook import VectorQuantizer, VectorQuantizerEMA
from .decoder import Decoder
from .encoder import Encoder
from .reparameterizer import DiagonalGaussian, reparameterize_kl

__all__ = ["Encoder", "Decoder", "DiagonalGaussian", "VectorQuantizer", "VectorQuantizerEMA", "reparameterize_kl"]
