"""``evaluate_autoencoder``: the reference's autoencoder ``_run_evaluate`` between building the model and writing
the CSVs (``src/pipelines/samplers/autoencoder_like.py:201-304``).

Per batch: reconstruct with ``reconstruct_vae_batch`` (timed between two device synchronisations, one model call
per batch, as the reference counts it), then ONE ``ops.image_metrics`` call WITHOUT the clamp (the reference
compares the reconstruction with the inputs as they are) and ONE host read of its ``[3, N]`` result.
"""
from __future__ import annotations

import time
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

from ...runtime import ops
from ...utils.model_utils.vae_utils import reconstruct_vae_batch
from ...utils.sampling_utils import append_eval_metrics, append_per_image_eval_metrics
from ..utils import sync_if_cuda
from ._rows import MetricTotals


def evaluate_autoencoder(model, cfg: Dict, batches: Iterable, device, *, metrics_root=None,
                         on_batch: Optional[Callable] = None) -> Tuple[Dict, List[Dict]]:
    """``batches`` yields ``(indices, samples)``; a sample is a dict with ``target`` and optionally ``img_id``,
    ``img_path``.  ``on_batch(indices, generated, targets)`` receives the device tensors.  Returns
    ``(summary_row, per_image_rows)``; with ``metrics_root`` the summary is appended to ``eval_metrics.csv``
    there and ``eval_metrics_per_image.csv`` is rewritten."""
    device = torch.device(device)
    recon_type = (cfg.get("training") or {}).get("recon_type", "l1")
    timing = {"model_seconds": 0.0, "model_calls": 0}
    totals = MetricTotals()
    for indices, samples in batches:
        targets = torch.stack([s["target"] for s in samples], dim=0).to(device)
        with torch.no_grad():
            sync_if_cuda(device)
            t0 = time.perf_counter()
            recon = reconstruct_vae_batch(model, targets, recon_type=recon_type)
            sync_if_cuda(device)
            timing["model_seconds"] += time.perf_counter() - t0
            timing["model_calls"] += 1
        recon, targets = recon.float().contiguous(), targets.float().contiguous()
        host = ops.image_metrics(recon, targets, clamp=False).stacked.cpu()
        totals.add_batch(indices, samples, host, has_ssim=recon.dim() >= 4)
        if on_batch is not None:
            on_batch(indices, recon, targets)
    row = totals.summary(timing)
    if metrics_root is not None:
        append_eval_metrics(metrics_root, row)
        append_per_image_eval_metrics(metrics_root, totals.rows)
    return row, totals.rows
