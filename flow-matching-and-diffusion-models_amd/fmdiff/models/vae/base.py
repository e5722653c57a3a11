"""``BaseVAE`` (reference ``src/models/vae/base.py:12-26``)."""
from __future__ import annotations

import abc

from ..autoencoder import BaseAutoencoder


class BaseVAE(BaseAutoencoder, metaclass=abc.ABCMeta):
    def make_discriminator(self):
        raise NotImplementedError("make_discriminator builds the MAGVIT discriminator only (VQVAE with "
                                  "discriminator_type='magvit'); for the PatchGAN stack construct "
                                  "fmdiff.nn.modules.vae.discriminators.PatchGANDiscriminatorND")
