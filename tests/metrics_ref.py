"""fp64 oracle and seeded input makers for the image-metrics kernel (csrc/metrics.hip, ops.image_metrics).

The oracle restates the definition, not the kernel: per image the mean of (g - t)^2, 10 log10(1 / max(mse, 1e-12)),
and skimage's structural_similarity defaults (uniform 7-wide window over every spatial axis, sample covariance,
C1 = 1e-4, C2 = 9e-4, the positions whose whole window lies inside the image), all in numpy float64 from the fp32
inputs, the window moments by DIRECT sums of the 7^ndim shifted slices.  test_metrics_ref.py holds it to a
scipy.ndimage.uniform_filter float64 restatement; test_gpu_metrics.py holds the kernel to it.

Bounds of the GPU tests ("Image metrics: fp64 bound"): |ssim - ssim64| <= 1e-9, mse within
1e-12 relative, psnr within 1e-9.
"""
import itertools

import numpy as np
import torch

WIN = 7
C1, C2 = 1e-4, 9e-4
SSIM_TOL = 1e-9
MSE_RTOL = 1e-12
PSNR_TOL = 1e-9
MAKERS = ("noisy", "flat_bright", "ct", "uniform", "identical", "out_of_range")


# ------------------------------------------------------------------ oracle
def window_mean(a):
    """Mean over every whole 7^ndim window of a float64 array, by direct sums of the shifted slices."""
    out = tuple(s - WIN + 1 for s in a.shape)
    acc = np.zeros(out, dtype=np.float64)
    for off in itertools.product(range(WIN), repeat=a.ndim):
        acc += a[tuple(slice(o, o + n) for o, n in zip(off, out))]
    return acc / float(WIN ** a.ndim)


def ssim_channel(x, y):
    """Mean SSIM of one channel (float64 arrays with two or three axes, every side >= 7)."""
    npix = float(WIN ** x.ndim)
    cov = npix / (npix - 1.0)
    ux, uy = window_mean(x), window_mean(y)
    vx = cov * (window_mean(x * x) - ux * ux)
    vy = cov * (window_mean(y * y) - uy * uy)
    vxy = cov * (window_mean(x * y) - ux * uy)
    s = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(s.mean())


def oracle(gen, tgt, clamp=True):
    """{"mse", "psnr", "ssim"}: float64 numpy [N] from two fp32 torch tensors [N, C, *spatial] (any device).
    ssim is NaN for [N, C, L] signals."""
    g, t = gen.detach().cpu().float(), tgt.detach().cpu().float()
    if clamp:
        g, t = g.clamp(0.0, 1.0), t.clamp(0.0, 1.0)    # torch.clamp: NaN stays NaN
    g, t = g.double().numpy(), t.double().numpy()
    n = g.shape[0]
    mse = ((g - t) ** 2).reshape(n, -1).mean(axis=1)
    with np.errstate(invalid="ignore"):
        psnr = 10.0 * np.log10(1.0 / np.maximum(mse, 1e-12))
    ssim = np.full((n,), np.nan)
    if g.ndim >= 4:
        for i in range(n):
            ssim[i] = np.mean([ssim_channel(g[i, c], t[i, c]) for c in range(g.shape[1])])
    return {"mse": mse, "psnr": psnr, "ssim": ssim}


def check(got, ref, what):
    """The three assertions of the GPU tests; ``got``: (mse, psnr, ssim) float64 sequences."""
    mse, psnr, ssim = (np.asarray(v, dtype=np.float64) for v in got)
    worst = {}
    for i in range(len(mse)):
        assert abs(mse[i] - ref["mse"][i]) <= MSE_RTOL * abs(ref["mse"][i]), \
            f"{what}[{i}]: mse {mse[i]!r} vs fp64 {ref['mse'][i]!r}"
        assert abs(psnr[i] - ref["psnr"][i]) <= PSNR_TOL, f"{what}[{i}]: psnr {psnr[i]!r} vs fp64 {ref['psnr'][i]!r}"
        if np.isnan(ref["ssim"][i]):
            assert np.isnan(ssim[i]), f"{what}[{i}]: ssim {ssim[i]!r}, expected NaN"
        else:
            assert abs(ssim[i] - ref["ssim"][i]) <= SSIM_TOL, f"{what}[{i}]: ssim {ssim[i]!r} vs fp64 {ref['ssim'][i]!r}"
            worst["ssim"] = max(worst.get("ssim", 0.0), abs(ssim[i] - ref["ssim"][i]))
        worst["psnr"] = max(worst.get("psnr", 0.0), abs(psnr[i] - ref["psnr"][i]))
        if ref["mse"][i]:
            worst["mse_rel"] = max(worst.get("mse_rel", 0.0), abs(mse[i] - ref["mse"][i]) / ref["mse"][i])
    return worst


# ------------------------------------------------------------------ input makers: (shape, seed) -> (gen, tgt) fp32
def _smooth(shape, g):
    """A smooth image in [0.15, 0.85]: a few low-frequency cosines per image and channel."""
    n, c, sp = shape[0], shape[1], shape[2:]
    grids = torch.meshgrid(*[torch.linspace(0.0, 1.0, s, dtype=torch.float64) for s in sp], indexing="ij")
    out = torch.zeros(shape, dtype=torch.float64)
    for i in range(n):
        for j in range(c):
            acc = torch.zeros(sp, dtype=torch.float64)
            for _ in range(3):
                k = torch.rand(len(sp), generator=g, dtype=torch.float64) * 2.5 + 0.5
                ph = torch.rand((), generator=g, dtype=torch.float64) * 6.283
                acc += torch.cos(sum(kk * 3.1416 * gg for kk, gg in zip(k, grids)) + ph)
            out[i, j] = 0.5 + 0.35 * acc / 3.0
    return out.float()


def make(kind, shape, seed=0):
    """A seeded (gen, tgt) pair of fp32 CPU tensors of ``shape`` = [N, C, *spatial]."""
    g = torch.Generator().manual_seed(1000 * MAKERS.index(kind) + seed)
    shape = tuple(shape)
    if kind == "noisy":                 # a smooth image plus 0.1 noise
        tgt = _smooth(shape, g)
        return tgt + 0.1 * torch.randn(shape, generator=g), tgt
    if kind == "flat_bright":           # 0.97 +- 1e-3: vx, vy, vxy are differences of nearly equal numbers
        return (0.97 + 1e-3 * torch.randn(shape, generator=g), 0.97 + 1e-3 * torch.randn(shape, generator=g))
    if kind == "ct":                    # exact zeros outside a thresholded region, in both images
        tgt = _smooth(shape, g)
        body = tgt > 0.5
        tgt = torch.where(body, tgt, torch.zeros(()))
        gen = torch.where(body, tgt + 0.05 * torch.randn(shape, generator=g), torch.zeros(()))
        return gen, tgt
    if kind == "uniform":               # independent images: SSIM near or below 0
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "identical":
        tgt = torch.rand(shape, generator=g)
        return tgt.clone(), tgt
    if kind == "out_of_range":          # values below 0 and above 1: the clamp matters
        return (1.6 * torch.rand(shape, generator=g) - 0.3, 1.6 * torch.rand(shape, generator=g) - 0.3)
    raise KeyError(kind)
