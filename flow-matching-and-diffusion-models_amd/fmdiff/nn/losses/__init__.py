"""Training losses (reference ``src/nn/losses``)."""
from .perceptual import VGGPerceptualLoss  # noqa: F401
from .vae import (PatchDiscriminator, PerceptualLoss, bce_focal_loss, discriminator_hinge_loss, focal_loss,  # noqa: F401
                  generator_hinge_loss, recon_loss, vq_regularizer)
