"""``compute_ssim_sample`` of the reference's ``src/utils/evaluation_utils.py:64-91``: SSIM of one sample in
channels-first layout, the mean of the per-channel values.

With ``ssim_fn=None`` the value comes from the HIP kernel (``ops.image_metrics``: skimage's defaults, all in
fp64) and the two tensors stay on the device; one host read returns the float.  With an ``ssim_fn`` (skimage's
``structural_similarity`` or a stand-in) the reference's host path runs: per channel
``ssim_fn(pred[c], tgt[c], channel_axis=None, data_range=1.0)`` on float32 numpy arrays.

``None`` under the reference's conditions: the shapes differ, fewer than two dimensions, or no channel with at
least two dimensions.  A two-dimensional sample is one ``[H, W]`` image, as in the reference.

The trainers' picture helpers of the same file (``:12-61``) are here too: ``latent_shape``, ``make_grid``,
``save_image`` and ``prepare_eval_batch``, with the reference's names and behaviour.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Callable, Optional, Tuple

import numpy as np
import torch

__all__ = ["compute_ssim_sample", "latent_shape", "make_grid", "save_image", "prepare_eval_batch"]


def latent_shape(vae_cfg: dict) -> Tuple[int, ...]:
    """``(embed_dim, *spatial)`` of the latent of a model config: ``resolution`` divided by 2 per level after the
    first (``down_channels`` if given, else ``ch_mult``), once per spatial dimension."""
    spatial_dims = vae_cfg.get("spatial_dims", 2)
    levels = vae_cfg.get("down_channels")
    if levels is None:
        levels = vae_cfg["ch_mult"]
    size = vae_cfg["resolution"] // 2 ** (len(tuple(levels)) - 1)
    return (vae_cfg["embed_dim"],) + (size,) * (spatial_dims if spatial_dims in (1, 3) else 2)


def make_grid(tensor: torch.Tensor, rows: int, cols: int) -> np.ndarray:
    """The first ``rows * cols`` images of ``[N, C, H, W]`` as one uint8 ``[rows H, cols W, 3 or C]`` array: clamp to
    [0, 1], one channel expanded to three, times 255, clipped and truncated."""
    n, c, h, w = tensor.shape
    if n < rows * cols:
        raise ValueError(f"Need at least {rows*cols} images to build the grid, found {n}")
    x = tensor[: rows * cols]
    if c == 1:
        x, c = x.expand(-1, 3, h, w), 3
    x = x.clamp(0.0, 1.0).reshape(rows, cols, c, h, w).permute(2, 0, 3, 1, 4).reshape(c, rows * h, cols * w)
    return (x.cpu().numpy() * 255.0).clip(0, 255).astype(np.uint8).transpose(1, 2, 0)


def save_image(array: np.ndarray, path) -> None:
    from PIL import Image
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(array).save(path)
    logging.info("Saved grid: %s", path)


def prepare_eval_batch(ds, count: int, device, seed: Optional[int] = None) -> torch.Tensor:
    """``count`` targets of ``ds`` chosen by ``select_visual_indices(ds, count, seed)``, stacked on ``device``."""
    from .model_utils.diffusion_utils import select_visual_indices
    if ds is None or len(ds) == 0:
        raise RuntimeError("Dataset is empty; cannot prepare evaluation batch.")
    tensors = [ds[i]["target"] for i in select_visual_indices(ds, count, seed=seed)]
    if not tensors:
        raise RuntimeError("Failed to collect evaluation samples.")
    return torch.stack(tensors, dim=0).to(device)


def compute_ssim_sample(pred: torch.Tensor, tgt: torch.Tensor, ssim_fn: Optional[Callable] = None) -> Optional[float]:
    if tuple(pred.shape) != tuple(tgt.shape) or pred.dim() < 2:
        return None
    if ssim_fn is None:
        from ..runtime import ops
        lead = (1, 1) if pred.dim() == 2 else (1,)
        g = pred.detach().float().reshape(*lead, *pred.shape).contiguous()
        t = tgt.detach().float().reshape(*lead, *tgt.shape).contiguous()
        return float(ops.image_metrics(g, t, clamp=False).ssim[0])
    p, t = pred.detach().cpu().float().numpy(), tgt.detach().cpu().float().numpy()
    if p.ndim == 2:
        return float(ssim_fn(p, t, channel_axis=None, data_range=1.0))
    scores = [float(ssim_fn(p[c], t[c], channel_axis=None, data_range=1.0)) for c in range(p.shape[0])
              if p[c].ndim >= 2]
    return sum(scores) / len(scores) if scores else None
