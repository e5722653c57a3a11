"""fp64 restatement and error bounds of the VAE criterion kernels (csrc/vae_loss.hip), shared by
test_vae_loss_bounds.py / test_vae_criterion.py (CPU) and test_gpu_vae_loss.py (GPU).  Every function runs on
the device of its inputs.  DESIGN.md section 4 ("VAE criterion: per-element bounds") carries the same derivation.

The kernel's stated arithmetic.  Inputs are fp32.  ``img = (clamp(x, -1, 1) + 1) * 0.5`` is three fp32 operations,
the ones torch performs, so ``img``, the clamp mask and ``sign(img - t)`` are decided on values both sides hold bit
for bit: no element is exempt from any check.  Everything after that is fp64, the transcendentals included, and
every value written is ONE rounding of its fp64 value to fp32.  With u = 2^-24 (round to nearest), v the fp64 value
and ``mag`` the sum of the magnitudes of the parts v is built from:

  element     |fl(v') - v| <= u |v| + K64 mag + TINY
              v' is the device's fp64 evaluation.  Its error is a handful of fp64 roundings and the device
              library's exp / log1p / expm1, documented at 1 ulp for double; K64 = 64 * 2^-53 (7e-15) allows 64 such
              half-ulps per element, about ten times what any path here makes, and is 1e-7 of the u term, so the
              margin cannot hide an fp32-sized error.  TINY = 2^-149 covers a result in the subnormal range.
              Every test prints observed / bound.
  gradient    dx = fl((g * scale / count) * unit): the same form with v = coef * unit, mag = |coef| mag_unit.
  sum         S = the fp64 sum of n values in a fixed order, then one division and one rounding:
              |fl(S / div) - L| <= u |L| + (n 2^-53 sum |v| + K64 sum mag) / div + TINY.

Against values recorded from the reference (fp32 torch on a CPU) the reference's own error is added
(``ref_*``): its element-wise roundings, counted per term below, and for a reduced value the worst case of an
fp32 sum of n terms, which holds for any order (pairwise, blocked or sequential): every partial sum is at most
sum |v| and each of the n - 1 additions rounds once, so |fl(sum) - sum| <= (n - 1) u sum |v| (1 + n u); the mean
adds one division, u |L|.
"""
import hashlib

import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
K64 = 64 * U64
TINY = 2.0 ** -149
TARGET_TERMS = ("l1", "mse", "bce", "focal", "bce_focal")
FREE_TERMS = ("hinge_real", "hinge_fake", "neg", "square")
TERMS = TARGET_TERMS + FREE_TERMS
REDUCTIONS = ("mean", "sum", "none")
ALPHA = 0.25


def gen(tag: str) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(int.from_bytes(hashlib.sha256(tag.encode()).digest()[:6], "little"))
    return g


def f2bf(x: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even bf16 of an fp32 tensor, as int16 bits."""
    return x.to(torch.bfloat16).view(torch.int16)


# ------------------------------------------------------------------ fp64 restatement of the terms
def img32(x: torch.Tensor) -> torch.Tensor:
    """raw_output_to_image for l1 / mse in fp32: torch's three operations."""
    return (x.clamp(-1.0, 1.0) + 1.0) * 0.5


def _logit_parts(x, t):
    e = torch.exp(-x.abs())
    r = 1.0 / (1.0 + e)
    pos = x >= 0
    sp, sn = torch.where(pos, r, e * r), torch.where(pos, e * r, r)
    lin = torch.where(x > 0, x * (1.0 - t), -x * t)      # max(x, 0) - x t
    l1p = torch.log1p(e)
    return sp, sn, lin + l1p, lin.abs() + l1p


def term64(term, x, t=None, alpha=ALPHA):
    """dict(v, u, mv, mu): the term and d term / dx in fp64 for fp32 ``x`` (and ``t``), with the magnitudes of
    their parts; autograd-differentiable in ``x64`` when ``x`` already is an fp64 leaf (test of the gradients)."""
    x64 = x.double() if x.dtype != torch.float64 else x
    if term in ("l1", "mse"):
        if x.dtype == torch.float64:       # the autograd check: the same formula without the fp32 detour
            img = (x64.clamp(-1.0, 1.0) + 1.0) * 0.5
            x32 = x64
        else:
            img, x32 = img32(x).double(), x
        d = img - t.double()
        m = ((x32 >= -1.0) & (x32 <= 1.0)).double()
        if term == "l1":
            return dict(v=d.abs(), u=torch.sign(d) * 0.5 * m, mv=d.abs(), mu=m)
        return dict(v=d * d, u=d * m, mv=d * d, mu=d.abs() * m)
    if term in ("bce", "focal", "bce_focal"):
        t64 = t.double()
        sp, sn, ce, mce = _logit_parts(x64, t64)
        v, u = torch.zeros_like(x64), torch.zeros_like(x64)
        mv, mu = torch.zeros_like(x64), torch.zeros_like(x64)
        if term != "focal":
            v, u, mv, mu = v + ce, u + (sp - t64), mv + mce, mu + sp + t64.abs()
        if term != "bce":
            q = t64 * sn + (1.0 - t64) * sp
            at = alpha * t64 + (1.0 - alpha) * (1.0 - t64)
            a, b = (q * q) * (sp - t64), 2.0 * q * sp * sn * (2.0 * t64 - 1.0) * ce
            v, u = v + at * (q * q) * ce, u + at * (a - b)
            mv, mu = mv + at.abs() * (q * q) * mce, mu + at.abs() * (a.abs() + b.abs())
        return dict(v=v, u=u, mv=mv, mu=mu)
    if term == "hinge_real":
        on = x64 < 1.0
        v = torch.where(on, 1.0 - x64, torch.zeros_like(x64))
        return dict(v=v, u=-on.double(), mv=v, mu=on.double())
    if term == "hinge_fake":
        on = x64 > -1.0
        v = torch.where(on, 1.0 + x64, torch.zeros_like(x64))
        return dict(v=v, u=on.double(), mv=v, mu=on.double())
    if term == "neg":
        return dict(v=-x64, u=-torch.ones_like(x64), mv=x64.abs(), mu=torch.ones_like(x64))
    if term == "square":
        return dict(v=x64 * x64, u=2.0 * x64, mv=x64 * x64, mu=2.0 * x64.abs())
    raise ValueError(term)


def _div(reduction, n):
    return float(n) if reduction == "mean" else 1.0


def loss64(term, x, t=None, reduction="mean", alpha=ALPHA):
    """(value, bound) of the kernel's loss output: a scalar for sum / mean, per element for none."""
    r = term64(term, x, t, alpha)
    if reduction == "none":
        return r["v"], U * r["v"].abs() + K64 * r["mv"] + TINY
    n, div = x.numel(), _div(reduction, x.numel())
    L = r["v"].sum() / div
    return L, U * L.abs() + (n * U64 * r["v"].abs().sum() + K64 * r["mv"].sum()) / div + TINY


def coef64(g, scale, reduction, n):
    """The fp64 coefficient the kernel forms from the fp32 upstream gradient and the fp32 scale."""
    g32 = torch.as_tensor(g, dtype=torch.float32)
    s32 = torch.tensor(scale, dtype=torch.float32).double().item()
    return g32.double() * s32 / _div(reduction, n)


def grad64(term, x, t=None, reduction="mean", g=1.0, scale=1.0, alpha=ALPHA):
    """(dx, bound) per element, in the shape of ``x``; ``g``: a number or an fp32 tensor of x's shape."""
    r = term64(term, x, t, alpha)
    c = coef64(g, scale, reduction, x.numel()).to(x.device)
    dx = c * r["u"]
    return dx, U * dx.abs() + K64 * c.abs() * r["mu"] + TINY


# ------------------------------------------------------------------ the reference's own fp32 error
def ref_sum_err(n, sum_abs):
    return (n - 1) * U * sum_abs * (1.0 + n * U)


def ref_term_err(term, x, t=None, alpha=ALPHA):
    """Bound of |reference fp32 term - exact term| per element.  Roundings counted on the reference's formulas:
    l1     img is shared; the subtraction and abs: 1.
    mse    the subtraction, the square: (1 + u)^2 on d^2 and one more rounding: 3.
    bce    binary_cross_entropy_with_logits evaluates (1 - t) x + max(-x, 0) + log(exp(-m) + exp(-x - m)): two
           products, three sums, exp and log at 1 ulp each, every one relative to a part no larger than |x| + 1: 8.
    focal  prob = sigmoid(x) (2 u absolute: 1 ulp of a value <= 1, twice for the reference's 1 - prob), p_t two
           products and a sum, 1 - p_t: dq = 8 u absolute on q = 1 - p_t; ce as above, dce = 8 u (|x| + 1);
           alpha_t 3 roundings, the square and two products 3 more:
           alpha_t ((2 q dq + dq^2) ce + q^2 dce) + 6 u |focal|.
    hinge  1 -+ x, relu: 1.   neg: 0 (exact).   square: 1."""
    r = term64(term, x, t, alpha)
    v = r["v"].abs()
    if term in ("l1", "hinge_real", "hinge_fake", "square"):
        return U * v
    if term == "neg":
        return torch.zeros_like(v)
    if term == "mse":
        return 3 * U * v
    x64, t64 = x.double(), t.double()
    e_bce = 8 * U * (x64.abs() + 1.0)
    if term == "bce":
        return e_bce
    sp, sn, ce, _ = _logit_parts(x64, t64)
    q = t64 * sn + (1.0 - t64) * sp
    at = (alpha * t64 + (1.0 - alpha) * (1.0 - t64)).abs()
    dq = 8 * U
    foc = at * (q * q) * ce
    e_foc = at * ((2 * q * dq + dq * dq) * ce + q * q * e_bce) + 6 * U * foc
    return e_foc if term == "focal" else e_foc + e_bce


def ref_loss_bound(term, x, t=None, reduction="mean", alpha=ALPHA, two_sums=False):
    """Bound of |recorded reference loss - exact loss|.  ``two_sums``: the reference reduced two tensors and added
    the results (bce_focal_loss, discriminator_hinge_loss): one more rounding."""
    r = term64(term, x, t, alpha)
    e = ref_term_err(term, x, t, alpha)
    if reduction == "none":
        return e + (U * r["v"].abs() if two_sums else 0.0)
    n, div = x.numel(), _div(reduction, x.numel())
    sum_abs = r["mv"].sum() + e.sum()
    L = (r["v"].sum() / div).abs()
    return (e.sum() + ref_sum_err(n, sum_abs)) / div + (2 + two_sums) * U * (L + sum_abs / div * U)


def ref_grad_err(term, x, t=None, reduction="mean", g=1.0, alpha=ALPHA):
    """Bound of |reference autograd gradient - exact gradient| per element, coef = g / count.
    The coefficient itself: g -> fp32, the division by n: 2 u.  Then, relative to |coef|:
    l1     sign * coef, * 0.5 (exact), * mask (exact): 1.       mse   2 d coef: the subtraction, two products: 3.
    hinge, neg: 0.   square: 2 x coef: 2.
    bce    (sigmoid(x) - t) coef: sigmoid 2 u absolute, the subtraction, the product: 4 u (1 + |t|).
    focal  autograd walks loss = a_t q^2 ce: d/dce = a_t q^2 and d/dq = 2 a_t q ce, each a few products (k = 16 u
           covers the longest chain: a_t 3, pow 2, products 3, the two branches of p_t 4, sigmoid' 3); q itself
           carries dq = 8 u absolute.  d q/d prob is formed as the SUM of g t and -g (1 - t), so its error is
           relative to |g|, not to |g (2t - 1)|:
           a_t [k u (2 q ce p (1-p) + q^2 (|p - t| + 1)) + dq (2 ce p (1-p) + 2 q |p - t|)]."""
    n = x.numel()
    c = coef64(g, 1.0, reduction, n).abs().to(x.device)
    r = term64(term, x, t, alpha)
    base = 2 * U * c * r["u"].abs()
    if term in ("l1", "hinge_real", "hinge_fake", "neg"):
        return base + U * c * r["u"].abs()
    if term == "mse":
        return base + 3 * U * c * r["mu"]
    if term == "square":
        return base + 2 * U * c * r["mu"]
    x64, t64 = x.double(), t.double()
    e_bce = 4 * U * c * (1.0 + t64.abs())
    if term == "bce":
        return base + e_bce
    sp, sn, ce, _ = _logit_parts(x64, t64)
    q = t64 * sn + (1.0 - t64) * sp
    at = (alpha * t64 + (1.0 - alpha) * (1.0 - t64)).abs()
    k, dq, pt = 16 * U, 8 * U, (sp - t64).abs()
    e_foc = c * at * (k * (2 * q * ce * sp * sn + q * q * (pt + 1.0)) + dq * (2 * ce * sp * sn + 2 * q * pt))
    return base + (e_foc if term == "focal" else e_foc + e_bce)


def vq_regularizer_ref64(latents):
    """The reference's formula (src/nn/losses/vae.py:121-126) in fp64: mean(mean_c^2) + mean((x - mean_c)^2)."""
    x = latents.double()
    dims = (0, *range(2, x.ndim))
    mean = x.mean(dim=dims, keepdim=True)
    return mean.pow(2).mean() + (x - mean).pow(2).mean()


# ------------------------------------------------------------------ posterior
def gauss64(moments_cf, eps=None):
    """fp64 restatement of the posterior on channels-first fp32 moments [N, 2E, *sp]: dict(z, kl, lv, s) with the
    kernel's bounds bz (per element) and bkl (per sample)."""
    mu32, raw = torch.chunk(moments_cf, 2, dim=1)
    lv = raw.clamp(-30.0, 20.0).double()      # the clamp is fp32 on both sides
    mu = mu32.double()
    s = torch.exp(0.5 * lv)
    ez = s * eps.double() if eps is not None else torch.zeros_like(mu)
    z = mu + ez
    dims = tuple(range(1, mu.ndim))
    em1 = torch.expm1(lv)
    terms = mu * mu + (em1 - lv)
    mag = mu * mu + em1.abs() + lv.abs()
    n = terms[0].numel()
    kl = 0.5 * terms.sum(dim=dims)
    bz = U * z.abs() + K64 * (mu.abs() + ez.abs()) + TINY if eps is not None else torch.zeros_like(z)
    bkl = U * kl.abs() + 0.5 * (n * U64 * terms.abs().sum(dim=dims) + K64 * mag.sum(dim=dims)) + TINY
    mask = ((raw >= -30.0) & (raw <= 20.0)).double()
    return dict(z=z, kl=kl, lv=lv, s=s, mu=mu, mask=mask, bz=bz, bkl=bkl, em1=em1)


def gauss_grad64(moments_cf, eps, g_z, g_kl):
    """(d_moments channels-first [N, 2E, *sp], bound): d_mu = g_z + g_kl mu, d_logvar = mask (g_z eps 0.5 s +
    g_kl 0.5 expm1(lv)); g_z / g_kl / eps None: zero."""
    r = gauss64(moments_cf, eps)
    mu, lv, s = r["mu"], r["lv"], r["s"]
    shape = [-1] + [1] * (mu.ndim - 1)
    gk = g_kl.double().view(shape) if g_kl is not None else torch.zeros([1] * mu.ndim, dtype=torch.float64,
                                                                        device=mu.device)
    gz = g_z.double() if g_z is not None else torch.zeros_like(mu)
    e = eps.double() if eps is not None else torch.zeros_like(mu)
    a, b = gz * e * 0.5 * s, gk * 0.5 * r["em1"]
    d = torch.cat([gz + gk * mu, r["mask"] * (a + b)], dim=1)
    mag = torch.cat([gz.abs() + (gk * mu).abs(), r["mask"] * (a.abs() + b.abs())], dim=1)
    return d, U * d.abs() + K64 * mag + TINY


def ref_gauss_err(moments_cf, eps):
    """The reference's fp32 error on (z, kl).  z: std = exp(0.5 lv) (the product is exact, exp 1 ulp, 1 rounding
    of std) 2 u; std * eps 1; the sum 1: 3 u |s eps| + u |z|.  kl: mu^2 1, var = exp(lv) 2, three additions each
    relative to a partial sum no larger than mu^2 + var + 1 + |lv|: 6 u of that per element; then an fp32 sum over
    the sample (ref_sum_err), the product by 0.5 exact."""
    r = gauss64(moments_cf, eps)
    mu, lv = r["mu"], r["lv"]
    ez = r["s"] * eps.double() if eps is not None else torch.zeros_like(mu)
    bz = 3 * U * ez.abs() + U * r["z"].abs()
    mag = mu * mu + torch.exp(lv) + 1.0 + lv.abs()
    dims = tuple(range(1, mu.ndim))
    n = mu[0].numel()
    e = 6 * U * mag
    bkl = 0.5 * (e.sum(dim=dims) + ref_sum_err(n, (mag + e).sum(dim=dims))) + U * r["kl"].abs()
    return bz, bkl


def ref_gauss_grad_err(moments_cf, eps, g_z, g_kl):
    """The reference's autograd error on d_moments.  g_kl = 0.7 / N: 2 u.  d_mu = g_z + 2 mu (0.5 g_kl): two
    products and the accumulation, 5 u (|g_z| + |g_kl mu|).  d_logvar accumulates g_z eps std 0.5 (exp's backward
    multiplies by the rounded std: 5 u) and the KL part as g var 0.5 plus -g 0.5 SEPARATELY, so its error is
    relative to |g_kl| 0.5 (var + 1), not to the difference: 5 u of each."""
    r = gauss64(moments_cf, eps)
    mu, lv, s = r["mu"], r["lv"], r["s"]
    shape = [-1] + [1] * (mu.ndim - 1)
    gk = g_kl.double().view(shape).abs()
    gz = g_z.double().abs() if g_z is not None else torch.zeros_like(mu)
    e = eps.double().abs() if eps is not None else torch.zeros_like(mu)
    d_mu = 5 * U * (gz + gk * mu.abs())
    d_lv = r["mask"] * 5 * U * (gz * e * 0.5 * s + gk * 0.5 * (torch.exp(lv) + 1.0))
    return torch.cat([d_mu, d_lv], dim=1)


# ------------------------------------------------------------------ checks
def check(name, got, want, bound, what):
    """Asserts |got - want| <= bound everywhere (a NaN on either side fails) and returns max(err / bound)."""
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=want.device).reshape(-1).expand_as(want)
    assert got.shape == want.shape, f"{name}: {what}: {tuple(got.shape)} against {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: {what}: not finite"
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    i = int(ratio.argmax())
    assert bool((err <= bound).all()), (f"{name}: {what}: error {float(err[i]):.3e} over bound {float(bound[i]):.3e} at "
                                        f"{i} (got {float(got[i])!r}, want {float(want[i])!r})")
    return float(ratio[i])


# ------------------------------------------------------------------ inputs with the planted kinks
def plant_rec(x, t):
    """rec at exactly +-1, just inside and just outside, and where img == target (in place on flat views)."""
    xf, tf = x.view(-1), t.view(-1)
    one = torch.tensor(1.0)
    inside, outside = torch.nextafter(one, torch.tensor(0.0)), torch.nextafter(one, torch.tensor(2.0))
    vals = [1.0, -1.0, float(inside), -float(inside), float(outside), -float(outside), 3.0, -3.0]
    for i, v in enumerate(vals):
        xf[i] = v
    k = len(vals)
    xf[k], xf[k + 1], xf[k + 2] = 0.25, 1.0, -1.5
    tf[k:k + 3] = img32(xf[k:k + 3])        # img == target: at an interior point, at the edge and outside
    return x, t


def plant_logits(x, t):
    """logits at +-100, +-5 and 0 against targets 0, 1 and soft."""
    xf, tf = x.view(-1), t.view(-1)
    i = 0
    for xv in (100.0, -100.0, 5.0, -5.0, 0.0):
        for tv in (0.0, 1.0, 0.3):
            xf[i], tf[i] = xv, tv
            i += 1
    return x, t


def plant_logvar(moments):
    """logvar (the second half of the channels) at -31, -30, 0, 20 and 21."""
    E = moments.shape[1] // 2
    half = moments[:, E:].contiguous()
    half.view(-1)[:5] = torch.tensor([-31.0, -30.0, 0.0, 20.0, 21.0], device=moments.device)
    moments[:, E:] = half
    return moments


def plant_disc(x):
    xf = x.view(-1)
    xf[0], xf[1], xf[2], xf[3] = 1.0, -1.0, 0.0, 2.5
    return x
