"""Seeded problems and the fp64 bounds shared by test_gpu_skip_bwd.py (GPU) and test_skip_bwd_bounds.py (CPU).

A skip-conv backward problem: dy [N][H][W][Kd], the block input x0|x1 [N][H][W][C0|C1], the GroupNorm-backward
operands dz [N][H][W][C], P/Q/R [N][C], the skip weights W_s [Kd][C], previous dx0/dx1 and previous dW/db.

The order bound.  dW_s[k][c] = sum_p dy[p][k] x[p][c] over M pixels.  The operands are bf16, so every product is
exact in fp32 (8 + 8 significand bits); two fp32 summations of the same M exact terms in different orders each
differ from the exact sum by at most (M - 1) u S + O(u^2), u = 2^-24, S = sum_p |dy x| (Higham, Accuracy and
Stability, eq. 4.4), so they differ from one another by less than 2 M u S.  The same holds for db with S = sum_p |dy|."""
import functools

import torch

U = 2.0 ** -24

# name -> (N, H, W, C0, C1, Kd)
CASES = {
    "c128_128": (2, 12, 12, 128, 128, 128),    # M = 288: tiles straddle the images, the last one is partial
    "c256_128": (2, 12, 12, 256, 128, 128),    # three c-tiles, the concat boundary on a tile boundary
    "k256": (2, 12, 12, 128, 0, 256),          # Kd = 256, single source: the plan refuses (c-tile not built)
    "single": (2, 12, 12, 128, 0, 128),        # taken, single source: x1 / dx1 are NULL
    "c192": (2, 12, 12, 128, 64, 128),         # taken, C = 192: the second c-tile is half empty
    "refused": (2, 12, 12, 64, 32, 64),        # Kd = 64: the plan refuses
    "g16": (2, 16, 16, 128, 128, 128),         # M = 512: the forced pixel-group counts
}


@functools.lru_cache(maxsize=None)
def problem(name):
    N, H, W, C0, C1, Kd = CASES[name]
    g = torch.Generator().manual_seed(4200 + sorted(CASES).index(name))
    C = C0 + C1
    bf = torch.bfloat16
    p = dict(N=N, H=H, W=W, C0=C0, C1=C1, Kd=Kd, M=N * H * W)
    p["dy"] = torch.randn(N, H, W, Kd, generator=g).to(bf)
    p["x0"] = torch.randn(N, H, W, C0, generator=g).to(bf)
    p["x1"] = torch.randn(N, H, W, C1, generator=g).to(bf) if C1 else None
    p["dz"] = torch.randn(N, H, W, C, generator=g).to(bf)
    p["P"] = torch.randn(N, C, generator=g)
    p["Q"] = torch.randn(N, C, generator=g) * 0.3
    p["R"] = torch.randn(N, C, generator=g) * 0.1
    p["w"] = torch.randn(Kd, C, 1, 1, generator=g) / C ** 0.5
    p["dx0"] = torch.randn(N, H, W, C0, generator=g).to(bf)
    p["dx1"] = torch.randn(N, H, W, C1, generator=g).to(bf) if C1 else None
    p["dw0"] = torch.randn(Kd, C, 1, 1, generator=g)
    p["db0"] = torch.randn(Kd, generator=g)
    return p


def flat(p):
    """dy [M][Kd], x [M][C] as fp64 (exact values of the bf16 operands)."""
    x = p["x0"] if p["x1"] is None else torch.cat([p["x0"], p["x1"]], -1)
    return p["dy"].double().reshape(p["M"], -1), x.double().reshape(p["M"], -1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 dW [Kd][C], db [Kd] and the sums of magnitudes S_w, S_b the bounds scale with."""
    dy, x = flat(problem(name))
    return dy.t() @ x, dy.sum(0), dy.abs().t() @ x.abs(), dy.abs().sum(0)


def order_bound(name):
    """(dW bound [Kd][C], db bound [Kd]): two differently ordered fp32 sums of the same exact products."""
    p = problem(name)
    _, _, Sw, Sb = reference(name)
    return 2 * p["M"] * U * Sw, 2 * p["M"] * U * Sb
