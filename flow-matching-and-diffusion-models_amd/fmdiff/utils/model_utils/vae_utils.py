"""``build_vae_model`` (reference ``src/utils/model_utils/vae_utils.py:14-51``): full config dict -> VAE on the
device through ``VAEFactory``, optional checkpoint.  Checkpoints are read with ``weights_only=True`` only.  The
batch encode / decode helpers of the reference live in ``fmdiff.pipelines.latent``; ``reconstruct_vae_batch``
(``:88-105``), the evaluate mode's encode + decode, is here."""
from __future__ import annotations

import contextlib
import warnings

import torch

from ...models.generators.vaefactory import VAEFactory

_RANDOM_INIT = r".*No checkpoint provided\. Random initialization\."


@contextlib.contextmanager
def _quiet_random_init():
    """The model constructors warn about random weights; here the caller may still load a checkpoint."""
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=_RANDOM_INIT)
        yield


def _config_names_checkpoint(cfg: dict) -> bool:
    named = (cfg.get("model") or {}).get("ckpt_path")
    return named is not None and not (isinstance(named, str) and named.lower() == "none")


def build_vae_model(cfg: dict, device: torch.device, ckpt_path=None, set_eval: bool = True):
    """``cfg`` is the loaded config with ``__config_path__`` (the factory reads the file itself); ``ckpt_path``: a
    state_dict or a ``{"model": state_dict}`` payload.  Warns once when an eval model ends up with random
    weights (no ``ckpt_path`` here and none in the config)."""
    if not cfg.get("__config_path__"):
        raise ValueError("Missing __config_path__ in config.")
    with _quiet_random_init():
        model = VAEFactory().build_from_json(cfg["__config_path__"]).to(device)
    if ckpt_path is not None:
        state = torch.load(ckpt_path, map_location=device, weights_only=True)
        if isinstance(state, dict) and "model" in state:
            state = state["model"]
        model.load_state_dict(state)
    if set_eval:
        model.eval()
        if ckpt_path is None and not _config_names_checkpoint(cfg):
            warnings.warn("[VAE] No checkpoint provided. Random initialization.")
    return model


def reconstruct_vae_batch(model, inputs: torch.Tensor, recon_type: str = "l1") -> torch.Tensor:
    """Encode + decode of image-space inputs in [0, 1], back in image space (reference ``vae_utils.py:88-105``):
    ``image_to_model_range`` -> forward with the posterior's mode -> ``raw_output_to_image``.  ``sample_posterior``
    is passed to the forwards that take it (AutoencoderKL); the VQ models have no posterior to sample."""
    import inspect
    x = model.image_to_model_range(inputs)
    takes = "sample_posterior" in inspect.signature(model.forward).parameters
    out = model(x, sample_posterior=False) if takes else model(x)
    if isinstance(out, (list, tuple)):
        out = out[0]
    return model.raw_output_to_image(out, recon_type=recon_type)
