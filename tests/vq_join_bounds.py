"""fp64 value and per-element error bound of the VQVAE latent join (csrc/vq_train.hip ``fmd_vq_join_bwd``,
``ops.vq_join_bwd``), shared by test_vq_join_bounds.py (CPU) and test_gpu_vq_join.py (GPU).  TEST INFRASTRUCTURE
ONLY.  DESIGN.md section 4 ("VQVAE trunk backward") carries the same derivation.

The kernel computes, per element of the first D channels of row m,

    out = bf16( fma( (g_loss * c) * scale , z - q , g ) ),      scale = 2 / (M D)

in fp32 with one final rounding to bf16 (nearest even); ``z - q`` is either formed there from fp32 z and the fp32
codebook row, or read as the saved fp32 residual (which is that same single rounding of z - q).  g is bf16 or fp32.

Exact value: ``v = g + s (z - q)`` with ``s = g_loss c 2 / (M D)`` (g_loss the fp32 scalar, c and 2/(MD) the host's
doubles), evaluated in fp64, whose own rounding (2^-53) is nine orders below the bound.

With u = 2^-24, the fp32 roundings on the path as the kernel is written are six:

    c -> fp32, 2/(MD) -> fp32, g_loss * c, that times scale         4, each relative to |s|, so 4 u |s (z - q)|
    z - q                                                           1, relative to |z - q|:       u |s (z - q)|
    the fma (one rounding of the exact coef * diff + g)             1, relative to the result:    u (|g| + |s (z - q)|)

so the fp32 result r obeys ``|r - v| <= B32 = 7 u (|g| + |s (z - q)|)``: six to first order, and k = 7 ("plus one", the
project's convention in tests/vq_train_bounds.py) covers the second-order terms.

The final rounding to bf16 (8 significant bits, to nearest) moves r by at most half a unit in its last place.  For
2^(e-1) <= |r| < 2^e that is 2^(e-9) = 2^-9 * 2^e: between 2^-9 |r| at the top of a binade and 2^-8 |r| at its
bottom, so ``2^-9 |v|`` alone is not a bound on a correctly rounded result (the emulation below exceeds it by up to a
factor two); the power of two takes the place of |v|.  With P(x) the smallest power of two above x, and |r| <= |v| + B32,

    |out - v| <= 2^-9 P(|v| + B32) + 7 * 2^-24 (|g| + |s (z - q)|)   (+ 2^-133, half the spacing of bf16
                                                                        subnormals, where a result underflows).

Padding channels (>= D) of the output are exact zeros and take no bound."""
from __future__ import annotations

import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -9
K_ROUNDINGS = 7
TINY = 2.0 ** -133
MUTANTS = ("g_rounded_to_bf16_first", "beta_for_classic", "truncate", "coef_in_bf16")


def coef64(g_loss: float, c: float, M: int, D: int) -> float:
    """s = g_loss c 2 / (M D) in double; ``g_loss`` is the value of the fp32 device scalar (None: zero)."""
    return 0.0 if g_loss is None else float(g_loss) * float(c) * 2.0 / (M * D)


def pow2_above(x: torch.Tensor) -> torch.Tensor:
    """P(x): the smallest power of two greater than x >= 0 (fp64; 0 for x = 0)."""
    _, e = torch.frexp(x)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e), torch.zeros_like(x))


def exact(g, z, q, s: float) -> torch.Tensor:
    """v = g + s (z - q) in fp64 for [M, D] operands; ``g`` None: zero; ``q`` None: ``z`` holds z - q."""
    diff = z.double() if q is None else z.double() - q.double()
    v = s * diff
    return v if g is None else v + g.double()


def bound(g, z, q, s: float) -> torch.Tensor:
    """The per-element bound on |out - v| of the module docstring."""
    diff = z.double() if q is None else z.double() - q.double()
    mag = (s * diff).abs()
    if g is not None:
        mag = mag + g.double().abs()
    b32 = K_ROUNDINGS * U32 * mag
    return UBF * pow2_above(exact(g, z, q, s).abs() + b32) + b32 + TINY


def emulate(g, z, q, g_loss, c: float, M: int, D: int, mutant=None) -> torch.Tensor:
    """The kernel's arithmetic in torch on the CPU: fp32 operations in its order, the fma as one rounding of the
    fp64 product-sum (exact for fp32 operands up to the final rounding), then bf16 nearest-even.  Returns fp32
    values on the bf16 grid.  ``mutant``: one of MUTANTS, a wrong kernel the bound has to catch."""
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    if mutant == "beta_for_classic":
        c = c + 1.0
    coef = (f32(0.0 if g_loss is None else g_loss) * f32(c)) * f32(2.0 / (M * D))
    if mutant == "coef_in_bf16":
        coef = coef.to(torch.bfloat16).float()
    diff = z.float() if q is None else z.float() - q.float()
    gg = torch.zeros_like(diff) if g is None else g.float()
    if mutant == "g_rounded_to_bf16_first":
        gg = gg.to(torch.bfloat16).float()
    r = (coef.double() * diff.double() + gg.double()).float()
    if mutant == "truncate":
        return (r.view(torch.int32) & -65536).view(torch.float32)
    return r.to(torch.bfloat16).float()


def check(name, got, v, bd):
    """Asserts |got - v| <= bd on every element (NaN fails); returns the largest error / bound."""
    err = (got.double() - v).abs()
    ok = err <= bd
    if not bool(ok.all()):
        worst = float(torch.nan_to_num(err / bd, nan=float("inf"))[~ok].max())
        raise AssertionError(f"{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bound (largest error / "
                             f"bound {worst:.3g})")
    return float((err / bd).max())


def bf16_valued(shape, gen: torch.Generator, scale: float = 1.0) -> torch.Tensor:
    """fp32 tensor of values that bf16 holds exactly."""
    return (scale * torch.randn(shape, generator=gen)).to(torch.bfloat16).float()


def make_case(M: int, D: int, K: int, seed: int):
    """Seeded CPU operands of one case: g [M, D] on the bf16 grid, z [M, D], the codebook [K, D], codes [M] and
    g_loss; magnitudes chosen so that g and s (z - q) are of the same order at the tests' M D."""
    gen = torch.Generator().manual_seed(seed)
    e = torch.randn((K, D), generator=gen)
    codes = torch.randint(0, K, (M,), generator=gen)
    z = e[codes] + 0.3 * torch.randn((M, D), generator=gen)
    g_loss = float(torch.tensor(0.37 * M * D).float())     # s (z - q) of the order of 0.1, like g
    g = bf16_valued((M, D), gen, 0.1)
    return g, z, e, codes, g_loss
