"""Row formatting shared by the two evaluate loops: the per-image rows and the summary row of the reference's
``_run_evaluate`` (``src/pipelines/samplers/diffusion_like.py:251-313``, ``autoencoder_like.py:243-298``)."""
from __future__ import annotations

from typing import Dict, List, Sequence

from ..utils import model_throughput


class MetricTotals:
    """Running sums of the per-image values (host floats, fp64) over the batches of one evaluation."""

    def __init__(self):
        self.mse = self.psnr = self.ssim = 0.0
        self.count = self.ssim_count = 0
        self.rows: List[Dict] = []

    def add_batch(self, indices: Sequence, samples: Sequence[Dict], host, has_ssim: bool = True) -> None:
        """``host``: the ``[3, N]`` (mse, psnr, ssim) result of one ``ops.image_metrics`` call, read to the host
        once.  ``has_ssim`` False (signals: no channel with two dimensions) is the reference's ``None``: an empty
        cell, left out of the SSIM mean."""
        mse, psnr, ssim = (host[k].tolist() for k in range(3))
        for j, sample_index in enumerate(indices):
            sample = samples[j]
            self.rows.append({"sample_index": sample_index, "img_id": sample.get("img_id"),
                              "img_path": sample.get("img_path"), "mse": f"{mse[j]:.8f}", "psnr": f"{psnr[j]:.6f}",
                              "ssim": f"{ssim[j]:.6f}" if has_ssim else ""})
            self.mse += mse[j]
            self.psnr += psnr[j]
            if has_ssim:
                self.ssim += ssim[j]
                self.ssim_count += 1
        self.count += len(mse)

    def summary(self, timing: Dict) -> Dict:
        """samples, mse, psnr, ssim, ssim_enabled, then ``model_throughput``'s fields."""
        if self.count == 0:
            raise RuntimeError("No samples available for evaluation.")
        row = {"samples": self.count, "mse": f"{self.mse / self.count:.8f}", "psnr": f"{self.psnr / self.count:.6f}",
               "ssim": f"{self.ssim / self.ssim_count:.6f}" if self.ssim_count else "", "ssim_enabled": True}
        row.update({k: v for k, v in model_throughput(timing, self.count).items() if k != "samples"})
        return row
