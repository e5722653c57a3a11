"""BatchNorm + LeakyReLU of the GAN discriminators (csrc/batchnorm.hip): fp64 restatement, per-output bounds, an
fp32 emulation of the kernels' operation order with mutants, and the whole-discriminator CPU oracle.

Imports without a GPU.  Notation: u = 2^-24 (fp32 unit roundoff), e64 = 2^-53, P(x) = the smallest power of two > x.
Convention ("GroupNorm: per-output bounds", "Quantizer training"): count the fp32 roundings on
the path of an output, add one, and take that many u relative to the sum of the absolute values of the terms.  A bf16
store moves the fp32 result r by at most half a bf16 ulp, 2^-9 P(|r|) (the latent-join section's power-of-two form):

    |out - v| <= 2^-9 P(|v| + B32) + B32            (B32: the bound on the fp32 result before the store)

Every stage is judged against the fp64 value of ITS OWN inputs (the slab, the fp32 a / b / mean / rstd it is given).

fmd_bn_fold (training).  The kernel adds the slab rows in fp64 (rows * e64, negligible but carried), forms
mean = S0/M and var = S1/M - mean^2 in fp64 and rounds each output once.
  mean        2u |mean| + slab_err sqrt(E[x^2])                             (1 rounding + 1)
  var         the subtraction cancels: an error d of the sums becomes d (E[x^2] + 2 mean^2) in var, so relative to
              var + eps it is amplified by  kappa = (E[x^2] + 2 mean^2) / (var + eps)  (|mean|/std = 8: kappa = 193).
              dvar = 16 e64 (E[x^2] + 2 mean^2) + slab_err (E[x^2] + 2 |mean| sqrt(E[x^2])); slab_err is the error
              the caller states for the sums themselves, relative to their sums of absolute terms (0 when the
              reference is the slab's own fp64 fold; E|x| <= sqrt(E[x^2]) stands in for the first sum's).
  rstd        2u rstd + rstd dvar / (2 (var + eps))
  a           2u |a| + |gamma| drstd          (gamma rstd in fp64, one rounding)
  b           2u (|beta| + |mean a|), against beta - mean a_f with the ROUNDED a_f the kernels multiply by (so an
              error of a does not reach a x + b twice)
  running_mean  3u (|(1-m) rm| + |m mean|)    (momentum arrives as fp32: 1, the store: 1, plus one)
  running_var   3u (|(1-m) rv| + |m var'|) + m M/(M-1) dvar,   var' = var M/(M-1)
  num_batches_tracked  exact (int64 + 1)
Eval mode: a, b, mean, rstd from the running statistics: the same rows with dvar = 16 e64 (rv + eps), kappa = 1.

fmd_bn_act_fwd.  r = fmaf(a, x, b) is ONE rounding of the exact a x + b, so sign(r) is the exact sign (rounding is
monotonic and a non-zero value does not round to zero): the branch of the LeakyReLU is the reference's branch at
every element, the kink included, and no element is left out.  On the negative side the slope arrives as fp32 (1) and
multiplies (1).  k = 3 + 1:
  y           B32 = 4u s (|a x| + |b|),  s = 1 for r > 0 and slope otherwise;  then the bf16 store.
Without a norm y = lrelu(x): B32 = 3u s |x|.

fmd_bn_act_bwd.  g = dy for r > 0, dy slope otherwise (2 roundings): dg = 2u |g|.  xhat = (x - mean) rstd (2
roundings): dxh = 2u (|x| + |mean|) rstd.  A lane adds its BN_ROWS/32 = 2 rows of a 64-row block in fp32, the 32 lanes
are added in order (a chain of K1 = 34 fp32 additions, the fma of sum g xhat rounding once per step like an add),
the blocks in fp64:
  S1 = sum g        E1 = (K1 + 2 + 1) u sum|g|
  S2 = sum g xhat   E2 = (K1 + 2 + 1) u sum|g xhat| + sum|g| dxh
  dbeta             E1 + 3u (|S1| + |old|)        (fp32(S1): 1, the fp32 +=: 1, plus one; old = 0 when stored)
  dgamma            E2 + 3u (|S2| + |old|)
  dx (training)     c1 = fp32(S1/M), c2 = fp32(S2/M);  t = g - c1 (1);  t = fmaf(-xhat, c2, t) (1);  dx = a t (1):
                    B32 = |a| [ 6u (|g| + |S1/M| + |xhat S2/M|) + (E1 + u|S1|)/M + (|xhat| (E2 + u|S2|) + dxh |S2|)/M ]
  dx (eval)         B32 = 4u |a g|          dx (no norm)   B32 = 3u |g|
then the bf16 store.  The derivative at r == 0 is ``slope`` (torch's leaky_relu backward tests r > 0).

Two-term forms (the walker's).  fmd_bn_act_fwd_split stores the fp32 result r as hi = bf16(r), lo = bf16(r - hi):
|r - hi| <= 2^-9 P(|r|), so P(|r - hi|) <= 2^-8 P(|r|) and the second store is within 2^-17 P(|r|):
  hi + lo     |hi + lo - v| <= 2^-17 P(|v| + B32) + B32        (hi itself: the bf16 store above)
x is then fp32; the counts above do not depend on x being a bf16 value, so fmd_bn_act_bwd_f32 keeps its rows.
fmd_bn_stats_f32: a slab entry is the reduce kernel's chain over one 64-row block, K1 additions (the square enters
through an fma: one rounding per step), plus one: (K1 + 1) u sum|x| and (K1 + 1) u sum x^2.

fmd_image_stage.  Mode 1: clamp is exact, +1 and * 0.5: B32 = 3u (|c| + 1)/2; mode 2: expf within 2 ulp, the add, the
division: B32 = 6u (s + |x| s (1 - s)); then the bf16 store.  Backward (fp32 out): mode 1 g/2 exact where
-1 <= x <= 1 (the boundary included, as torch.clamp), 0 elsewhere; mode 2: s (1 - s) is formed as e / (1 + e)^2 with
e = exp(-|x|), which has no 1 - s cancellation: expf (2), 1 + e (1, entering twice: 2), the square (1), the division
(1), the product with g (1), plus one: 8u |g s (1 - s)|.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
E64 = 2.0 ** -53
BF16 = torch.bfloat16
F64 = torch.float64
BN_ROWS = 64
K1 = BN_ROWS // 32 + 32
SLOPE = 0.2
MAX_MEAN_OVER_STD = 8.0   # the inputs' largest |mean| / std per channel


def pow2_above(x):
    """The smallest power of two strictly greater than x (elementwise, fp64); 0 for x == 0."""
    x = x.double()
    e = torch.floor(torch.log2(x.clamp_min(1e-300))) + 1
    p = torch.pow(torch.tensor(2.0, dtype=F64), e)
    p = torch.where(p <= x, p * 2, p)
    return torch.where(x > 0, p, torch.zeros_like(p))


def bf16_store(v, b32):
    """Bound on |out - v| of a bf16 store whose fp32 value is within b32 of v."""
    return 2.0 ** -9 * pow2_above(v.abs() + b32) + b32


def split_store(v, b32):
    """Bound on |hi + lo - v| of the two-term store of an fp32 value within b32 of v."""
    return 2.0 ** -17 * pow2_above(v.abs() + b32) + b32


def emulate_split(r):
    """(hi, lo) bf16 of an fp32 tensor, as split8 forms them."""
    hi = r.to(BF16)
    return hi, (r - hi.float()).to(BF16)


def stats_f32_ref(x, rows=BN_ROWS):
    """fp64 (slab [blocks][C][2], bound) of fmd_bn_stats_f32 on an fp32 [M][C] tensor."""
    M, C = x.shape
    nb = -(-M // rows)
    xb = torch.cat([x.double(), torch.zeros(nb * rows - M, C, dtype=F64)]).reshape(nb, rows, C)
    ref = torch.stack([xb.sum(1), (xb * xb).sum(1)], -1)
    bound = (K1 + 1) * U * torch.stack([xb.abs().sum(1), (xb * xb).sum(1)], -1)
    return ref, bound


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(M, C, seed, with_norm=True):
    """x, dy bf16 [M][C]; gamma, beta, running statistics fp32.  Channel c has mean_c / std_c spread over
    [-MAX_MEAN_OVER_STD, MAX_MEAN_OVER_STD]; dy has a non-zero mean (so that sum g / M matters)."""
    g = torch.Generator().manual_seed(seed)
    ratio = torch.linspace(-MAX_MEAN_OVER_STD, MAX_MEAN_OVER_STD, C, dtype=F64)
    std = torch.rand(C, generator=g, dtype=F64) + 0.5
    x = (torch.randn(M, C, generator=g, dtype=F64) * std + ratio * std).to(BF16)
    dy = (torch.randn(M, C, generator=g, dtype=F64) * 0.5 + 0.25).to(BF16)
    T = dict(x=x, dy=dy)
    T["gamma"] = (torch.rand(C, generator=g) + 0.5).float()
    T["beta"] = (torch.randn(C, generator=g) * 0.3).float()
    T["rm"] = (torch.randn(C, generator=g) * 0.5).float()
    T["rv"] = (torch.rand(C, generator=g) + 0.5).float()
    T["old_dgamma"] = torch.randn(C, generator=g).float()
    T["old_dbeta"] = torch.randn(C, generator=g).float()
    return T


def plant_kink(x, a, b):
    """Make u = a x + b exactly 0 at a few elements: in channel 0 set a = 0.5, b = -1 (caller's a, b are changed in
    place) and x[0..2][0] = 2, and put one element on each side of the kink next to them."""
    a[0], b[0] = 0.5, -1.0
    x[0:3, 0] = 2.0
    x[3, 0], x[4, 0] = 4.0, 1.0   # u = 1 and u = -0.5
    return x


def kink_census(x, a, b):
    u = a.double() * x.double() + b.double()
    return int((u == 0).sum()), int((u > 0).sum()), int((u < 0).sum())


def slab_of(x, rows=BN_ROWS):
    """[ceil(M/rows)][C][2] fp32: each entry the correctly rounded fp64 sum of its rows (relative error u)."""
    M, C = x.shape
    xd = x.double()
    nb = -(-M // rows)
    pad = torch.zeros(nb * rows - M, C, dtype=F64)
    xb = torch.cat([xd, pad]).reshape(nb, rows, C)
    return torch.stack([xb.sum(1), (xb * xb).sum(1)], -1).float()


# ------------------------------------------------------------------------------------- fp64 restatement
def fold_ref(slab, M, gamma, beta, rm, rv, eps=1e-5, momentum=0.1, training=True):
    """fp64: dict(a, b, mean, rstd, rm, rv, var, ex2)."""
    gamma, beta, rm, rv = (t.double() for t in (gamma, beta, rm, rv))
    if training:
        S = slab.double().sum(0)
        mean = S[:, 0] / M
        ex2 = S[:, 1] / M
        var = (ex2 - mean * mean).clamp_min(0)
        rm2 = (1 - momentum) * rm + momentum * mean
        rv2 = (1 - momentum) * rv + momentum * var * (M / (M - 1))
    else:
        mean, var, ex2, rm2, rv2 = rm, rv, rv + rm * rm, rm, rv
    rstd = 1 / torch.sqrt(var + eps)
    a = gamma * rstd
    return dict(a=a, b=beta - mean * a, mean=mean, rstd=rstd, rm=rm2, rv=rv2, var=var, ex2=ex2)


def fold_bounds(R, M, gamma, beta, rm, rv, a_got, eps=1e-5, momentum=0.1, training=True, slab_err=0.0):
    """Bounds for the outputs of fold_ref's dict ``R``; ``a_got``: the fp32 a the kernel stored (b is built on it)."""
    gamma, beta, rm, rv = (t.double() for t in (gamma, beta, rm, rv))
    mean, var, rstd = R["mean"], R["var"], R["rstd"]
    ax = torch.sqrt(R["ex2"])   # E|x| <= sqrt(E[x^2])
    dvar = (16 * E64 * (R["ex2"] + 2 * mean * mean) + slab_err * (R["ex2"] + 2 * mean.abs() * ax) if training
            else 16 * E64 * (var + eps))
    drstd = 2 * U * rstd + rstd * dvar / (2 * (var + eps))
    da = 2 * U * R["a"].abs() + gamma.abs() * drstd
    b_ref = beta - mean * a_got.double()
    B = dict(mean=2 * U * mean.abs() + slab_err * ax, rstd=drstd, a=da,
             b=2 * U * (beta.abs() + (mean * R["a"]).abs()) + 16 * E64)
    if training:
        unb = var * (M / (M - 1))
        B["rm"] = 3 * U * (((1 - momentum) * rm).abs() + (momentum * mean).abs())
        B["rv"] = 3 * U * (((1 - momentum) * rv).abs() + momentum * unb) + momentum * (M / (M - 1)) * dvar
    return B, b_ref


def kappa(R, eps=1e-5):
    """The cancellation factor of E[x^2] - mean^2 per channel."""
    return (R["ex2"] + 2 * R["mean"] ** 2) / (R["var"] + eps)


def act_fwd_ref(x, a, b, slope=SLOPE):
    """fp64 (v, B32): the value and the fp32 bound before the bf16 store."""
    xd = x.double()
    if a is None:
        r = xd
        terms = xd.abs()
        k = 3
    else:
        r = a.double() * xd + b.double()
        terms = (a.double() * xd).abs() + b.double().abs()
        k = 4
    s = torch.where(r > 0, torch.ones_like(r), torch.full_like(r, slope))
    return r * s, k * U * s * terms


def act_bwd_ref(dy, x, a, b, mean, rstd, M, slope=SLOPE, training=True, old_dgamma=None, old_dbeta=None):
    """fp64 restatement of the backward: dict(dx, dgamma, dbeta, g, xhat, S1, S2)."""
    dyd, xd = dy.double(), x.double()
    if a is None:
        g = torch.where(xd > 0, dyd, dyd * slope)
        return dict(dx=g, g=g)
    a, b, mean, rstd = (t.double() for t in (a, b, mean, rstd))
    r = a * xd + b
    g = torch.where(r > 0, dyd, dyd * slope)
    xh = (xd - mean) * rstd
    S1, S2 = g.sum(0), (g * xh).sum(0)
    dx = a * (g - S1 / M - xh * S2 / M) if training else a * g
    og = 0 if old_dgamma is None else old_dgamma.double()
    ob = 0 if old_dbeta is None else old_dbeta.double()
    return dict(dx=dx, dgamma=S2 + og, dbeta=S1 + ob, g=g, xhat=xh, S1=S1, S2=S2)


def act_bwd_bounds(R, x, a, mean, rstd, M, training=True, old_dgamma=None, old_dbeta=None):
    """dict(dx, dgamma, dbeta): bounds on |out - R[...]|; dx includes the bf16 store."""
    g = R["g"]
    if a is None:
        return dict(dx=bf16_store(R["dx"], 3 * U * g.abs()))
    a, mean, rstd = (t.double() for t in (a, mean, rstd))
    xh, S1, S2 = R["xhat"], R["S1"], R["S2"]
    dxh = 2 * U * (x.double().abs() + mean.abs()) * rstd
    E1 = (K1 + 3) * U * g.abs().sum(0)
    E2 = (K1 + 3) * U * (g * xh).abs().sum(0) + (g.abs() * dxh).sum(0)
    og = 0 if old_dgamma is None else old_dgamma.double().abs()
    ob = 0 if old_dbeta is None else old_dbeta.double().abs()
    out = dict(dbeta=E1 + 3 * U * (S1.abs() + ob), dgamma=E2 + 3 * U * (S2.abs() + og))
    if training:
        b32 = a.abs() * (6 * U * (g.abs() + (S1 / M).abs() + (xh * S2 / M).abs()) + (E1 + U * S1.abs()) / M +
                         (xh.abs() * (E2 + U * S2.abs()) + dxh * S2.abs()) / M)
    else:
        b32 = 4 * U * (a * g).abs()
    out["dx"] = bf16_store(R["dx"], b32)
    return out


def image_ref(x, mode):
    """fp64 (value, B32) of the image map: 0 identity, 1 (clamp + 1) / 2, 2 sigmoid."""
    xd = x.double()
    if mode == 0:
        return xd, torch.zeros_like(xd)
    if mode == 1:
        c = xd.clamp(-1, 1)
        return (c + 1) / 2, 3 * U * (c.abs() + 1) / 2
    s = torch.sigmoid(xd)
    return s, 6 * U * (s + xd.abs() * s * (1 - s))


def image_bwd_ref(g, x, mode):
    """fp64 (value, bound) of the gradient to the raw x from the bf16 gradient g (fp32 output)."""
    gd, xd = g.double(), x.double()
    if mode == 0:
        return gd, torch.zeros_like(gd)
    if mode == 1:
        return torch.where((xd >= -1) & (xd <= 1), gd * 0.5, torch.zeros_like(gd)), torch.zeros_like(gd)
    s = torch.sigmoid(xd)
    v = gd * s * (1 - s)
    return v, 8 * U * v.abs()


# ------------------------------------------------------------------------- fp32 emulation of the kernels
def _fma32(a, x, b):
    """fmaf on fp32 tensors: the product of an fp32 and a bf16-valued or fp32 operand and the sum are exact enough
    in fp64 (<= 48 + guard bits), rounded once to fp32."""
    return (a.double() * x.double() + b.double()).float()


def emulate_fold(slab, M, gamma, beta, rm, rv, eps=1e-5, momentum=0.1, training=True, mutant=None):
    """The kernel's arithmetic: fp64 fold, outputs rounded once.  Returns dict(a, b, mean, rstd, rm, rv) fp32."""
    mom = float(torch.tensor(momentum, dtype=torch.float32))
    if training:
        S = slab.double().sum(0)
        mean = S[:, 0] / M
        var = (S[:, 1] / M - mean * mean).clamp_min(0)
        rstd = 1 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
        unb = var if mutant == "biased_running_var" else var * (M / (M - 1.0))
        if mutant == "momentum_wrong_side":
            rm2 = (mom * rm.double() + (1 - mom) * mean).float()
            rv2 = (mom * rv.double() + (1 - mom) * unb).float()
        else:
            rm2 = ((1 - mom) * rm.double() + mom * mean).float()
            rv2 = ((1 - mom) * rv.double() + mom * unb).float()
    else:
        mean = rm.double()
        rstd = 1 / torch.sqrt(rv.double() + float(torch.tensor(eps, dtype=torch.float32)))
        rm2, rv2 = rm.clone(), rv.clone()
    a = (gamma.double() * rstd).float()
    if mutant == "a_bf16":
        a = a.to(BF16).float()
    b = (beta.double() - mean * a.double()).float()
    return dict(a=a, b=b, mean=mean.float(), rstd=rstd.float(), rm=rm2, rv=rv2)


def emulate_fwd(x, a, b, slope=SLOPE, split=False):
    sl = torch.tensor(slope, dtype=torch.float32)
    r = x.float() if a is None else _fma32(a, x, b)
    r = torch.where(r > 0, r, r * sl)
    return emulate_split(r) if split else r.to(BF16)


def _block_sum(v):
    """The reduce kernel's order for [M][C] fp32 terms: lane pl adds rows pl, pl + 32 of each 64-row block, the 32
    lanes are added in ascending order, the blocks in fp64."""
    M, C = v.shape
    nb = -(-M // BN_ROWS)
    vb = torch.cat([v, torch.zeros(nb * BN_ROWS - M, C)]).reshape(nb, BN_ROWS // 32, 32, C)
    lane = torch.zeros(nb, 32, C)
    for j in range(BN_ROWS // 32):
        lane = lane + vb[:, j]
    tot = lane[:, 0].clone()
    for p in range(1, 32):
        tot = tot + lane[:, p]
    return tot.double().sum(0)


def _block_fma_sum(g, xh):
    M, C = g.shape
    nb = -(-M // BN_ROWS)
    z = torch.zeros(nb * BN_ROWS - M, C)
    gb = torch.cat([g, z]).reshape(nb, BN_ROWS // 32, 32, C)
    hb = torch.cat([xh, z]).reshape(nb, BN_ROWS // 32, 32, C)
    lane = torch.zeros(nb, 32, C)
    for j in range(BN_ROWS // 32):
        lane = _fma32(gb[:, j], hb[:, j], lane)
    tot = lane[:, 0].clone()
    for p in range(1, 32):
        tot = tot + lane[:, p]
    return tot.double().sum(0)


def emulate_bwd(dy, x, a, b, mean, rstd, M, slope=SLOPE, training=True, old_dgamma=None, old_dbeta=None,
                mutant=None, running=None):
    """The kernels' arithmetic in fp32 (reduce, fp64 fold, apply).  Returns dict(dx bf16, dgamma, dbeta fp32).
    ``running``: (mean, rstd) of the running statistics for the ``xhat_from_running`` mutant."""
    sl = torch.tensor(slope, dtype=torch.float32)
    dyf, xf = dy.float(), x.float()
    if a is None:
        return dict(dx=torch.where(xf > 0, dyf, dyf * sl).to(BF16))
    r = _fma32(a, x, b)
    pos = r > 0
    if mutant == "derivative_0_at_kink":
        g = torch.where(pos, dyf, torch.where(r == 0, torch.zeros_like(dyf), dyf * sl))
    elif mutant == "derivative_1_at_kink":
        g = torch.where(r >= 0, dyf, dyf * sl)
    else:
        g = torch.where(pos, dyf, dyf * sl)
    mu, rs = (mean, rstd) if mutant != "xhat_from_running" else running
    xh = (xf - mu) * rs
    S1, S2 = _block_sum(g), _block_fma_sum(g, xh)
    out = {}
    out["dbeta"] = S1.float() if old_dbeta is None else old_dbeta + S1.float()
    out["dgamma"] = S2.float() if old_dgamma is None else old_dgamma + S2.float()
    if training:
        c1, c2 = (S1 / M).float(), (S2 / M).float()
        if mutant == "no_mean_term":
            c1 = torch.zeros_like(c1)
        out["dx"] = (a * _fma32(-xh, c2, g - c1)).to(BF16)
    else:
        out["dx"] = (a * g).to(BF16)
    return out


def ratio(got, ref, bound):
    """max |got - ref| / bound (elements with a zero bound must be exact)."""
    err = (got.double() - ref).abs()
    z = bound <= 0
    if bool((err[z] > 0).any()):
        return math.inf
    return float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0


# ---------------------------------------------------------------------------- whole-discriminator oracle
MAGVIT_TABLE = ((1, 4, 2, 1, True), (2, 4, 2, 1, True), (4, 4, 2, 1, True), (8, 4, 1, 1, True), (0, 4, 1, 0, False))
PATCHGAN_TABLE = ((1, 4, 2, 1, True), (2, 4, 2, 1, True), (4, 4, 2, 1, True), (8, 4, 2, 1, True), (0, 3, 1, 1, False))
TABLES = {"magvit": MAGVIT_TABLE, "patchgan": PATCHGAN_TABLE}


class _BnAct(torch.autograd.Function):
    """BatchNorm2d + LeakyReLU by the closed forms above (fold_ref / act_fwd_ref / act_bwd_ref) on NCHW tensors, in
    the dtype of its input; returns (y, new running_mean, new running_var)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, rm, rv, training, eps, momentum, slope):
        N, C, H, W = y.shape
        M = N * H * W
        f = y.permute(0, 2, 3, 1).reshape(M, C)
        if training:
            mean = f.mean(0)
            var = (f * f).mean(0) - mean * mean if y.dtype == F64 else f.var(0, unbiased=False)
            rm2 = (1 - momentum) * rm + momentum * mean
            rv2 = (1 - momentum) * rv + momentum * var * (M / (M - 1))
        else:
            mean, var, rm2, rv2 = rm, rv, rm, rv
        rstd = 1 / torch.sqrt(var + eps)
        a = gamma * rstd
        b = beta - mean * a
        r = a * f + b
        ctx.save_for_backward(f, a, mean, rstd, r)
        ctx.meta = (training, slope, (N, C, H, W))
        out = torch.where(r > 0, r, r * slope)
        return out.reshape(N, H, W, C).permute(0, 3, 1, 2), rm2, rv2

    @staticmethod
    def backward(ctx, gout, *_):
        f, a, mean, rstd, r = ctx.saved_tensors
        training, slope, (N, C, H, W) = ctx.meta
        M = N * H * W
        dy = gout.permute(0, 2, 3, 1).reshape(M, C)
        g = torch.where(r > 0, dy, dy * slope)
        xh = (f - mean) * rstd
        S1, S2 = g.sum(0), (g * xh).sum(0)
        dx = a * (g - S1 / M - xh * S2 / M) if training else a * g
        return dx.reshape(N, H, W, C).permute(0, 3, 1, 2), S2, S1, None, None, None, None, None, None


def disc_keys(table):
    """[(conv key prefix, norm key prefix or None)] in the Sequential's numbering."""
    keys, i = [], 0
    for li, (mult, ks, stride, pad, act) in enumerate(table):
        norm = act and li > 0
        keys.append((f"model.{i}.conv", f"model.{i + 1}" if norm else None))
        i += 1 + int(norm) + int(act)
    return keys


def disc_oracle(sd, table, x, training=True, dtype=torch.float32, slope=SLOPE, eps=1e-5, momentum=0.1):
    """Logits and the buffers after the pass, by torch on the CPU in ``dtype``: F.conv2d plus the closed-form
    BatchNorm + LeakyReLU node.  ``sd`` values may require grad (cast to ``dtype`` by the caller)."""
    h = x
    bufs = {}
    for (mult, ks, stride, pad, act), (ck, nk) in zip(table, disc_keys(table)):
        h = F.conv2d(h, sd[ck + ".weight"], sd[ck + ".bias"], stride=stride, padding=pad)
        if nk is not None:
            h, rm2, rv2 = _BnAct.apply(h, sd[nk + ".weight"], sd[nk + ".bias"], sd[nk + ".running_mean"].to(dtype),
                                       sd[nk + ".running_var"].to(dtype), training, eps, momentum, slope)
            bufs[nk + ".running_mean"], bufs[nk + ".running_var"] = rm2.detach(), rv2.detach()
            bufs[nk + ".num_batches_tracked"] = sd[nk + ".num_batches_tracked"] + int(training)
        elif act:
            h = F.leaky_relu(h, slope)
    return h, bufs


def oracle_params(sd, dtype):
    """Leaf copies of the floating state_dict entries in ``dtype`` (parameters require grad)."""
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            out[k] = v.clone()
        elif "running_" in k:
            out[k] = v.detach().to(dtype)
        else:
            out[k] = v.detach().to(dtype).clone().requires_grad_()
    return out
