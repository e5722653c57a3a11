"""fp64 restatement of the latent 1x1 conv backward (csrc/pointwise_bwd.hip, ``ops.pointwise_bwd``) and the error
bound its GPU test uses.  TEST INFRASTRUCTURE ONLY.

The kernel: ``dy`` and ``x`` are bf16, ``W`` is fp32.  Every product is formed in fp64, where it is exact (8 x 8
and 8 x 24 significant bits), every sum is an fp64 sum of such products in some fixed order, and every output is one
rounding of that sum to fp32:

    g[m][e]  = fl32(sum_z dy[m][z] W[z][e])        Z terms
    dW[z][e] = fl32(sum_m dy[m][z] x[m][e])        M terms
    db[z]    = fl32(sum_m dy[m][z])                M terms

so with ``v`` the exact value, ``u = 2^-53`` and ``gamma_n = n u / (1 - n u)`` (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2: any order of summation of n terms)

    |got - v| <= 2^-24 |v| + gamma_n sum |terms|.

With ``accumulate`` the rounded value is added in fp32 to the value ``old`` already there, one more rounding:
``|got - (old + v)| <= b + 2^-24 (|old + v| + b)`` with ``b`` the bound above.

``exact`` computes ``v`` with ``math.fsum`` over the exact fp64 products, i.e. correctly rounded."""
from __future__ import annotations

import math

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n: int) -> float:
    return n * U64 / (1.0 - n * U64)


def kernel_fp64(dy: torch.Tensor, x: torch.Tensor, W: torch.Tensor):
    """The kernel's arithmetic before its final roundings, in fp64 with the sums in ascending order.
    ``dy`` [M, >= Z], ``x`` [M, >= E] (bf16-valued), ``W`` [Z, E].  Returns (g [M, E], dW [Z, E], db [Z])."""
    Z, E = W.shape
    d, xx, w = dy[:, :Z].double(), x[:, :E].double(), W.double()
    g = torch.zeros((d.shape[0], E), dtype=torch.float64)
    for z in range(Z):
        g = g + d[:, z:z + 1] * w[z:z + 1, :]
    dW = torch.zeros((Z, E), dtype=torch.float64)
    db = torch.zeros((Z,), dtype=torch.float64)
    for m in range(d.shape[0]):
        dW = dW + d[m, :, None] * xx[m, None, :]
        db = db + d[m]
    return g, dW, db


def exact(dy: torch.Tensor, x: torch.Tensor, W: torch.Tensor):
    """Correctly rounded fp64 values and the sums of the absolute terms:
    ((g, dW, db), (g_abs, dW_abs, db_abs)) as fp64 tensors."""
    Z, E = W.shape
    d, xx, w = dy[:, :Z].double(), x[:, :E].double(), W.double()
    M = d.shape[0]
    pg = (d[:, :, None] * w[None, :, :]).permute(0, 2, 1).contiguous()      # [M, E, Z], exact products
    g = torch.tensor([[math.fsum(r) for r in row] for row in pg.tolist()], dtype=torch.float64).reshape(M, E)
    pw = (d[:, :, None] * xx[:, None, :]).permute(1, 2, 0).contiguous()     # [Z, E, M]
    dW = torch.tensor([[math.fsum(r) for r in row] for row in pw.tolist()], dtype=torch.float64).reshape(Z, E)
    db = torch.tensor([math.fsum(r) for r in d.t().contiguous().tolist()], dtype=torch.float64)
    return (g, dW, db), (pg.abs().sum(-1), pw.abs().sum(-1), d.abs().sum(0))


def bound(v: torch.Tensor, abs_terms: torch.Tensor, n: int, old: torch.Tensor = None) -> torch.Tensor:
    """The per-element bound on ``|got - v|`` (``|got - (old + v)|`` with ``old``, the accumulate case)."""
    b = U32 * v.abs() + gamma(n) * abs_terms
    if old is not None:
        b = b + U32 * ((old.double() + v).abs() + b)
    return b


def bf16_valued(shape, gen: torch.Generator, scale: float = 1.0) -> torch.Tensor:
    """fp32 tensor of values that bf16 holds exactly."""
    return (scale * torch.randn(shape, generator=gen)).to(torch.bfloat16).float()
