"""Evaluate loops of the reference's ``src/pipelines/samplers``: sample or reconstruct every batch, score it on
the device (``ops.image_metrics``) and format the metrics rows."""
from .autoencoder_like import evaluate_autoencoder
from .diffusion_like import evaluate_diffusion

__all__ = ["evaluate_autoencoder", "evaluate_diffusion"]
