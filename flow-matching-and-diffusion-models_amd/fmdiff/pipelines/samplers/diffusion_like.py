"""``evaluate_diffusion``: what the reference's ``_run_evaluate`` does between building the model and writing the
CSVs (``src/pipelines/samplers/diffusion_like.py:202-319``), on the HIP engine.

Per batch: stack the targets, take the conditioning from ``image`` when the mode is ``concatenate`` or
``attention`` (and every sample has one), sample with ``decode_diffusion_batch``, then ONE
``ops.image_metrics`` call (the clamp to [0, 1] of both tensors is inside the kernel) and ONE host read of its
``[3, N]`` result.  Dataset construction, run directories, saved images and the CLI are the caller's.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

from ...runtime import ops
from ...utils.model_utils import diffusion_utils as DU
from ...utils.sampling_utils import append_eval_metrics, append_per_image_eval_metrics
from ..utils import resolve_conditioning_mode
from ._rows import MetricTotals


def evaluate_diffusion(model, cfg: Dict, batches: Iterable, device, *, num_inference_steps: Optional[int] = None,
                       start_step: Optional[int] = None, last_n_steps: Optional[int] = None,
                       scheduler: Optional[str] = None, metrics_root=None,
                       on_batch: Optional[Callable] = None) -> Tuple[Dict, List[Dict]]:
    """``batches`` yields ``(indices, samples)``; a sample is a dict with ``target`` and optionally ``image``,
    ``img_id``, ``img_path``.  ``scheduler``: a ``run_model --scheduler`` alias overriding the config's.
    ``on_batch(indices, generated, targets)`` receives the device tensors as sampled (the metrics clamp a copy
    in registers, not these).  Returns ``(summary_row, per_image_rows)``; with ``metrics_root`` the summary is
    appended to ``eval_metrics.csv`` there and ``eval_metrics_per_image.csv`` is rewritten."""
    training_cfg, model_cfg = cfg["training"], cfg["model"]
    mode = resolve_conditioning_mode(training_cfg.get("conditioning") or model_cfg.get("conditioning"))
    timing = {"model_seconds": 0.0, "model_calls": 0}
    totals = MetricTotals()
    for indices, samples in batches:
        targets = torch.stack([s["target"] for s in samples], dim=0).to(device)
        cond = None
        if mode in {"concatenate", "attention"}:
            images = [s.get("image") for s in samples]
            if all(c is not None for c in images):
                cond = torch.stack(images, dim=0).to(device)
        with torch.no_grad():
            generated = DU.decode_diffusion_batch(
                model, training_cfg, model_cfg, device, targets.shape, cond, timing=timing,
                num_inference_steps=num_inference_steps, start_step=start_step, last_n_steps=last_n_steps,
                reference_batch=targets, init_from_reference=(start_step is not None) or (last_n_steps is not None),
                scheduler_override=scheduler)
        generated, targets = generated.float().contiguous(), targets.float().contiguous()
        host = ops.image_metrics(generated, targets, clamp=True).stacked.cpu()
        totals.add_batch(indices, samples, host, has_ssim=generated.dim() >= 4)
        if on_batch is not None:
            on_batch(indices, generated, targets)
    row = totals.summary(timing)
    if metrics_root is not None:
        append_eval_metrics(metrics_root, row)
        append_per_image_eval_metrics(metrics_root, totals.rows)
    return row, totals.rows
