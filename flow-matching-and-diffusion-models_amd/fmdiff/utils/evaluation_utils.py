"""``compute_ssim_sample`` of the reference's ``src/utils/evaluation_utils.py:64-91``: SSIM of one sample in
channels-first layout, the mean of the per-channel values.

With ``ssim_fn=None`` the value comes from the HIP kernel (``ops.image_metrics``: skimage's defaults, all in
fp64) and the two tensors stay on the device; one host read returns the float.  With an ``ssim_fn`` (skimage's
``structural_similarity`` or a stand-in) the reference's host path runs: per channel
``ssim_fn(pred[c], tgt[c], channel_axis=None, data_range=1.0)`` on float32 numpy arrays.

``None`` under the reference's conditions: the shapes differ, fewer than two dimensions, or no channel with at
least two dimensions.  A two-dimensional sample is one ``[H, W]`` image, as in the reference.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch


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
