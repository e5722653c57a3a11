"""VAE modules (reference ``src/nn/modules/vae/__init__.py``): encoder, decoder, diagonal Gaussian and the
vector-quantizer codebooks (``csrc/vq.hip``, ``csrc/vq_train.hip``) and the GAN discriminators
(``discriminators``, ``csrc/batchnorm.hip``)."""
from .codebook import VectorQuantizer, VectorQuantizerEMA
from .decoder import Decoder
from .discriminators import MagvitDiscriminator, MagvitDiscriminatorND, PatchGANDiscriminatorND
from .encoder import Encoder
from .reparameterizer import DiagonalGaussian, reparameterize_kl

__all__ = ["Encoder", "Decoder", "DiagonalGaussian", "VectorQuantizer", "VectorQuantizerEMA", "reparameterize_kl",
           "MagvitDiscriminator", "MagvitDiscriminatorND", "PatchGANDiscriminatorND"]
