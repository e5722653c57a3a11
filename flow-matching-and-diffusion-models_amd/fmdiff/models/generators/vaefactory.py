"""``VAEFactory`` (reference ``src/models/generators/vaefactory.py:16-97``): a JSON config's ``model`` block ->
``AutoencoderKL`` (``latent_type: "kl"``, the default) or ``VQVAE`` (``"vq"``), with the reference's key
normalisation and error texts, so ``configs/*vae*.json`` and ``configs/*vqvae*.json`` are drop-in.

``norm_type`` / ``act`` reach the residual blocks through the block factory as in the reference; the engine
fuses GroupNorm + SiLU only, so any other pair raises ``NotImplementedError`` when the blocks are built."""
from __future__ import annotations

import functools
import json
import os
from typing import Any, Dict

from ...nn.blocks.residual import ResBlockND
from ..vae.kl import AutoencoderKL
from ..vae.vq import VQVAE

__all__ = ["VAEFactory", "build_from_json"]

LATENT_TYPES = {"kl": AutoencoderKL, "vq": VQVAE}
# read by the factory itself; the model constructors do not take them
SELECTORS = ("model_type", "latent_type", "norm_type", "act")
# JSON writes a missing value of these as the string "None"
NULLABLE = ("emb_channels", "ckpt_path", "down_channels")


def _read_model_block(json_path) -> Dict[str, Any]:
    json_path = os.fspath(json_path)
    if not os.path.exists(json_path):
        raise FileNotFoundError(f"Config not found: {json_path}")
    with open(json_path) as f:
        doc = json.load(f)
    if "model" not in doc:
        raise ValueError("Config must contain a 'model' section.")
    return dict(doc["model"])


def _none_string(v) -> bool:
    return isinstance(v, str) and v.lower() == "none"


class VAEFactory:
    def __init__(self) -> None:
        self._model_registry = dict(LATENT_TYPES)

    def build_from_json(self, json_path):
        block = _read_model_block(json_path)
        kind = str(block.get("model_type", "vae")).lower()
        if kind != "vae":
            raise ValueError(f"Expected model_type 'vae', got '{kind}'.")
        latent = block.get("latent_type", "kl").lower()
        if latent not in self._model_registry:
            raise ValueError(f"Unsupported latent_type '{latent}'. Expected one of {list(self._model_registry)}.")
        args = {k: (None if k in NULLABLE and _none_string(v) else v) for k, v in block.items() if k not in SELECTORS}
        if isinstance(args.get("down_channels"), list):
            args["down_channels"] = tuple(args["down_channels"])
        args.setdefault("in_channels", 3)
        args.setdefault("out_channels", args["in_channels"])
        args.setdefault("resolution", 256)
        # norm / activation preferences travel with every residual block the encoder and decoder make
        args["block_factory"] = functools.partial(ResBlockND, norm_type=block.get("norm_type", "gn"),
                                                  act=block.get("act", "silu"))
        return self._model_registry[latent](**args)


def build_from_json(json_path):
    return VAEFactory().build_from_json(json_path)
