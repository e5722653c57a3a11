"""The VGG perceptual loss kernels (csrc/perceptual.hip): fp64 restatement, per-output bounds, an fp32 emulation of
the kernels' arithmetic with mutants, and the whole-loss CPU oracle ``perc_oracle``.

Imports without a GPU.  Notation and convention as tests/bn_bounds.py: u = 2^-24, e64 = 2^-53, P(x) the smallest power
of two > x; count the fp32 roundings on the path of an output, add one, and take that many u relative to the sum of
the absolute values of the terms; a bf16 store is 2^-9 P(|v| + B32) + B32 and a two-term store (hi = bf16(r),
lo = bf16(r - hi)) is 2^-17 P(|v| + B32) + B32.  Every stage is judged against the fp64 value of ITS OWN inputs.

Each kernel is restated ONCE, parametrised by the dtype: in fp64 it is the reference, in fp32 (every torch operation
rounding once, as the kernel's) it is the emulation, and the emulation takes a ``mutant`` that breaks one rule.

The reference's own class (src/nn/losses/vae.py PerceptualLoss) cannot be recorded as a golden on a machine without
torchvision: it then returns 0 for every input.  So the oracle here is written from the formulae of the issue
(F.interpolate(bilinear, align_corners=False), Conv2d, ReLU, MaxPool2d(2, 2), mean |a - b|), the way
``bn_bounds.disc_oracle`` was, and the closed forms below are checked against torch autograd in fp64.

The bilinear axis.  Destination o of an axis of ``n_in`` source pixels reads i0 = floor(s), i1 = min(i0 + 1, n_in - 1)
with s = max((o + 1/2) n_in / n_out - 1/2, 0) and weights 1 - l, l, l = s - i0.  A resize is A_h X A_w^T with the
[n_out][n_in] matrices of those weights, and its gradient A_h^T G A_w: the gather the backward kernel runs.  The
kernel forms scale = fp32(n_in) / fp32(n_out) (1), the product (1) and the subtraction (1): with one more,
    ds(o) = 4u ((o + 1/2) n_in / n_out + 1/2)
bounds the error of s; l = s - i0 (1) and 1 - l (1) add 2u.  The interpolant is continuous and piecewise linear in s,
so where the rounded s falls on the other side of an integer the value still moves by at most ds times the local
differences; the bound therefore takes |x| over the widened window i0 - 1 .. i1 + 1:
    dl(o) = ds(o) + 2u,        coordinate term = dl(o) sum_{i in window} |x_i|.

fmd_perc_stage.  v = l0y (l0x a + l1x b) + l1y (l0x c + l1x d): a product (1), the add (1), a product (1), the add (1)
on every path, plus one: 5u sum |weights| |x|, plus the coordinate terms of both axes, plus the image map's own error
carried through |A_h| . |A_w|^T (clamp map 3u (|c| + 1)/2, sigmoid 6u (s + |x| s (1 - s)): bn_bounds); then the
two-term store.  Without a resize only the map and the store remain.

fmd_perc_stage_bwd.  gs = (g0 + g1) + g2 for one repeated channel (2), the edge weight l0 + l1 (1), wy wx (1), the
product with gs (1), and a chain of n additions over the n = n_y n_x readers of the source pixel (n), plus one:
(n + 6) u sum |w| |g|, plus the coordinate terms, then the map's derivative: clamp exact (x 1/2 or 0), sigmoid
8u |g s (1 - s)| (bn_bounds).  The output is fp32.

fmd_perc_tap_fwd.  relu of an fp32 value is exact, and r - t is ONE rounding of the exact difference, so its sign is
the exact sign and |r - t| is within u |r - t|: no element is left out at any kink.  The sum is fp64 over n elements
(n e64), the division fp64, the result rounded once: with one more
    |value - ref| <= (3u + n e64) ref.
loss <- loss + w value is a product (1) and an add (1) per tap: 3u (|loss| + |w value|) accumulated.  sgn is exact.
The operand is relu(max of the window), exact in fp32: B32 = 0, the two-term store only.

fmd_perc_tap_bwd.  coef = fp32(g w / count) from fp64 arithmetic: 2u |coef|; coef sgn is exact, the add with the
gradient from below (1), plus one:  B32 = [y > 0] (2u |coef sgn| + 2u (|coef sgn| + |below|)),  then the bf16 store.
The derivative of the ReLU at y == 0 is 0, sign(0) = 0, and the pool sends its gradient to the FIRST maximum of the
window in row-major order; pixels the floor leaves outside every window get the L1 term only.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from bn_bounds import U, E64, BF16, F64, bf16_store, split_store  # noqa: F401

F32 = torch.float32
IMAGE_MODES = ("identity", "clamp", "sigmoid")
NARROW = (8, 8, "M", 16, 16, "M", 24, 24, 24, "M", 40, 40, 40)
VGG16 = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512)
MUTANTS = ("pool_last_max", "relu_grad_at_zero", "sign_zero_is_one", "divisor_padded", "align_corners", "no_half_pixel",
           "no_edge_clamp", "grad_to_target_half", "weights_reversed")


# ---------------------------------------------------------------------------------------------- the bilinear axis
def axis_matrix(n_out: int, n_in: int, dtype=F64, mutant: str = ""):
    """[n_out][n_in] interpolation weights of one axis in ``dtype`` arithmetic (each operation one rounding)."""
    o = torch.arange(n_out, dtype=dtype)
    if mutant == "align_corners":
        s = o * (torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(max(n_out - 1, 1), dtype=dtype))
    else:
        scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
        s = o * scale if mutant == "no_half_pixel" else (o + 0.5) * scale - 0.5
    s = s.clamp_min(0)
    i0 = s.long().clamp_max(n_in - 1)
    i1 = i0 + 1 if mutant == "no_edge_clamp" else torch.where(i0 < n_in - 1, i0 + 1, i0)
    l1 = s - i0.to(dtype)
    l0 = 1 - l1
    A = torch.zeros(n_out, n_in + 1, dtype=dtype)   # column n_in: past the edge (read as nothing)
    rows = torch.arange(n_out)
    A[rows, i0] += l0
    A[rows, i1] += l1
    return A[:, :n_in].contiguous()


def axis_bound(n_out: int, n_in: int):
    """(dl [n_out], window [n_out][n_in] 0/1): the error of the weights and the widened window they act on."""
    o = torch.arange(n_out, dtype=F64)
    p = (o + 0.5) * n_in / n_out
    dl = 4 * U * (p + 0.5) + 2 * U
    s = (p - 0.5).clamp_min(0)
    i0 = s.long().clamp_max(n_in - 1)
    idx = torch.arange(n_in)
    win = ((idx[None, :] >= (i0 - 1)[:, None]) & (idx[None, :] <= (i0 + 2)[:, None])).double()
    return dl, win


def image_map(x, mode: str):
    if mode == "clamp":
        return (x.clamp(-1, 1) + 1) * 0.5
    if mode == "sigmoid":
        return 1 / (1 + torch.exp(-x))
    return x


def image_map_bound(x, mode: str):
    x = x.double()
    if mode == "clamp":
        return 3 * U * (x.clamp(-1, 1).abs() + 1) / 2
    if mode == "sigmoid":
        s = torch.sigmoid(x)
        return 6 * U * (s + x.abs() * s * (1 - s))
    return torch.zeros_like(x)


def image_map_grad(x, mode: str):
    if mode == "clamp":
        return ((x >= -1) & (x <= 1)).to(x.dtype) * 0.5
    if mode == "sigmoid":
        e = torch.exp(-x.abs())
        return e / ((1 + e) * (1 + e))
    return torch.ones_like(x)


# ---------------------------------------------------------------------------------------------- staging
def stage(recon, target, mode="identity", size=None, dtype=F64, mutant: str = ""):
    """v [2 N][Ho][Wo][8] in ``dtype``: what fmd_perc_stage stores as hi + lo (recon first, channels 3..7 zero)."""
    N, C, Hs, Ws = recon.shape
    x = torch.cat([image_map(recon.to(dtype), mode), target.to(dtype)])
    if size is not None and tuple(size) != (Hs, Ws):
        Ah, Aw = axis_matrix(size[0], Hs, dtype, mutant), axis_matrix(size[1], Ws, dtype, mutant)
        x = torch.einsum("oi,ncij,pj->ncop", Ah, x, Aw)
    if C == 1:
        x = x.expand(-1, 3, -1, -1)
    v = torch.zeros(2 * N, x.shape[2], x.shape[3], 8, dtype=dtype)
    v[..., :3] = x.permute(0, 2, 3, 1)
    return v


def stage_bound(recon, target, mode="identity", size=None):
    """Bound on |hi + lo - stage(fp64)|, [2 N][Ho][Wo][8]."""
    N, C, Hs, Ws = recon.shape
    xm = torch.cat([image_map(recon.double(), mode), target.double()]).abs()
    bm = torch.cat([image_map_bound(recon, mode), torch.zeros_like(target, dtype=F64)])
    if size is not None and tuple(size) != (Hs, Ws):
        Ah, Aw = axis_matrix(size[0], Hs).abs(), axis_matrix(size[1], Ws).abs()
        (dh, wh), (dw, ww) = axis_bound(size[0], Hs), axis_bound(size[1], Ws)
        b32 = 5 * U * torch.einsum("oi,ncij,pj->ncop", Ah, xm, Aw)
        b32 = b32 + torch.einsum("oi,ncij,pj->ncop", dh[:, None] * wh, xm, Aw + ww * dw[:, None])
        b32 = b32 + torch.einsum("oi,ncij,pj->ncop", Ah, xm, dw[:, None] * ww)
        b32 = b32 + torch.einsum("oi,ncij,pj->ncop", Ah, bm, Aw)
        xm = torch.einsum("oi,ncij,pj->ncop", Ah, xm, Aw)
    else:
        b32 = bm
    if C == 1:
        xm, b32 = xm.expand(-1, 3, -1, -1), b32.expand(-1, 3, -1, -1)
    out = torch.zeros(2 * N, xm.shape[2], xm.shape[3], 8, dtype=F64)
    out[..., :3] = split_store(xm, b32).permute(0, 2, 3, 1)
    return out


def stage_bwd(g, recon, mode="identity", dtype=F64, mutant: str = ""):
    """dx [N][C][Hs][Ws] in ``dtype`` from g [N][Ho][Wo][Cp] (bf16 values)."""
    N, C, Hs, Ws = recon.shape
    Ho, Wo = g.shape[1], g.shape[2]
    gd = g.to(dtype)
    gs = ((gd[..., 0] + gd[..., 1]) + gd[..., 2])[:, None] if C == 1 else gd[..., :3].permute(0, 3, 1, 2)
    if (Ho, Wo) != (Hs, Ws):
        Ah, Aw = axis_matrix(Ho, Hs, dtype, mutant), axis_matrix(Wo, Ws, dtype, mutant)
        gs = torch.einsum("oi,ncop,pj->ncij", Ah, gs, Aw)
    return gs * image_map_grad(recon.to(dtype), mode)


def stage_bwd_bound(g, recon, mode="identity"):
    N, C, Hs, Ws = recon.shape
    Ho, Wo = g.shape[1], g.shape[2]
    gd = g.double().abs()
    ga = (gd[..., 0] + gd[..., 1] + gd[..., 2])[:, None] if C == 1 else gd[..., :3].permute(0, 3, 1, 2)
    d = image_map_grad(recon.double(), mode).abs()
    if (Ho, Wo) != (Hs, Ws):
        Ah, Aw = axis_matrix(Ho, Hs).abs(), axis_matrix(Wo, Ws).abs()
        (dh, wh), (dw, ww) = axis_bound(Ho, Hs), axis_bound(Wo, Ws)
        # readers of a source pixel; + 2 per axis: a rounded coordinate may add one reader at either end
        n = ((Ah > 0).sum(0) + 2)[:, None] * ((Aw > 0).sum(0) + 2)[None, :]
        s = torch.einsum("oi,ncop,pj->ncij", Ah, ga, Aw)
        b = (n + 6) * U * s
        b = b + torch.einsum("oi,ncop,pj->ncij", dh[:, None] * wh, ga, Aw + ww * dw[:, None])
        b = b + torch.einsum("oi,ncop,pj->ncij", Ah, ga, dw[:, None] * ww)
    else:
        s = ga
        b = 3 * U * s
    b = b * d
    if mode == "sigmoid":
        b = b + 8 * U * s * d
    return b


# ---------------------------------------------------------------------------------------------- tap
def _windows(y):
    """[N][Ho][Wo][C][4] view of the complete 2x2 windows of y [N][H][W][C], k = 2 dy + dx."""
    N, H, W, C = y.shape
    Ho, Wo = H // 2, W // 2
    w = y[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C)
    return w.permute(0, 1, 3, 5, 2, 4).reshape(N, Ho, Wo, C, 4)


def tap_fwd(y, C: int, pool: bool, dtype=F64, mutant: str = ""):
    """y [2 N][H][W][Cp] fp32 -> (value in fp64 / as the kernel's fp32, sgn int8 [N][H][W][Cp], operand
    [2 N][h][w][Cp] (relu, pooled with ``pool``) in ``dtype``)."""
    N2, H, W, Cp = y.shape
    N = N2 // 2
    yd = y.to(dtype).clone()
    yd[..., C:] = 0
    r, t = yd[:N].clamp_min(0), yd[N:].clamp_min(0)
    d = r - t
    count = N * (Cp if mutant == "divisor_padded" else C) * H * W
    value = d.abs().double().sum() / count
    if dtype != F64:
        value = value.to(dtype)
    sgn = torch.sign(d)
    if mutant == "sign_zero_is_one":
        sgn = torch.where(d == 0, torch.ones_like(d), sgn)
    sgn[..., C:] = 0
    if pool:
        out = _windows(yd).max(-1).values.clamp_min(0)
    else:
        out = yd.clamp_min(0)
    return value, sgn.to(torch.int8), out


def tap_value_bound(y, C: int, ref_value):
    N2, H, W, _ = y.shape
    return (3 * U + (N2 // 2) * C * H * W * E64) * float(ref_value)


def tap_out_bound(out_ref):
    return split_store(out_ref.double().abs(), torch.zeros_like(out_ref, dtype=F64))


def tap_bwd(y_rec, sgn, C: int, g_loss: float, weight: float, g_below=None, pool: bool = False, dtype=F64,
            mutant: str = ""):
    """dy [2 N][H][W][Cp] in ``dtype``; the target half is NaN (untouched).  ``weight`` and ``g_loss`` are taken as
    the fp32 values the kernel receives."""
    N, H, W, Cp = y_rec.shape
    count = float(N) * C * H * W
    coef = float(torch.tensor(g_loss, dtype=F32)) * float(torch.tensor(weight, dtype=F32)) / count
    coef = torch.tensor(coef, dtype=dtype)   # fp32: the kernel's one rounding
    y = y_rec.to(dtype)
    below = torch.zeros(N, H, W, Cp, dtype=dtype)
    if g_below is not None:
        gb = g_below.to(dtype)
        if pool:
            w = _windows(y)
            best, arg = w[..., 0], torch.zeros(w.shape[:-1], dtype=torch.long)
            for k in range(1, 4):
                upd = w[..., k] >= best if mutant == "pool_last_max" else w[..., k] > best
                arg = torch.where(upd, torch.full_like(arg, k), arg)
                best = torch.where(upd, w[..., k], best)
            Ho, Wo = H // 2, W // 2
            routed = torch.zeros(N, Ho, Wo, Cp, 4, dtype=dtype).scatter_(-1, arg[..., None], gb[..., None])
            routed = routed.reshape(N, Ho, Wo, Cp, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, Cp)
            below[:, :2 * Ho, :2 * Wo] = routed
        else:
            below = gb
    alive = y >= 0 if mutant == "relu_grad_at_zero" else y > 0
    l1 = coef * sgn.to(dtype)
    dy = torch.where(alive, l1 + below, torch.zeros_like(below))
    full = torch.full((2 * N, H, W, Cp), float("nan"), dtype=dtype)
    full[:N] = dy
    if mutant == "grad_to_target_half":
        full[N:] = dy
    parts = dict(l1=l1.double().abs() * alive, below=below.double().abs() * alive)
    return full, parts


def tap_bwd_bound(ref_full, parts):
    N = ref_full.shape[0] // 2
    b32 = 2 * U * parts["l1"] + 2 * U * (parts["l1"] + parts["below"])
    return bf16_store(ref_full[:N].double(), b32)


def lattice_y(N: int, H: int, W: int, Cp: int, C: int, seed: int):
    """A tapped conv output [2 N][H][W][Cp] on the lattice k / 4, |k| <= 12, that holds every kink: y = 0 exactly,
    r = t exactly (both dead, and both alive and equal), elements on both sides, and positive ties inside pool
    windows (few distinct values).  Non-zero |r - t| >= 1/4 >= 2^-20.  Padding channels are zero."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(-12, 13, (2 * N, H, W, Cp), generator=g).float() / 4
    same = torch.rand(N, H, W, Cp, generator=g) < 0.2
    y[N:] = torch.where(same, y[:N], y[N:])          # r == t: dead pairs and alive, equal pairs
    zero = torch.rand(2 * N, H, W, Cp, generator=g) < 0.1
    y = torch.where(zero, torch.zeros_like(y), y)    # y == 0 exactly
    if H >= 2 and W >= 2:
        y[0, 0, 0, 0] = y[0, 0, 1, 0] = y[0, 1, 0, 0] = y[0, 1, 1, 0] = 1.0      # [[1, 1], [1, 1]] -> element 0
        y[0, 0, 0, 1], y[0, 0, 1, 1], y[0, 1, 0, 1], y[0, 1, 1, 1] = 0.0, 2.0, 2.0, 2.0   # [[0, 2], [2, 2]] -> 1
    y[..., C:] = 0
    return y


def loss_fold(values, weights, dtype=F64, mutant: str = ""):
    """loss = w_0 v_0, then loss + w_k v_k in tap order, each operation in ``dtype``; (loss, sum |w v|)."""
    ws = list(weights)[::-1] if mutant == "weights_reversed" else list(weights)
    loss, mag = None, 0.0
    for v, w in zip(values, ws):
        t = torch.tensor(float(torch.tensor(w, dtype=F32)), dtype=dtype) * torch.as_tensor(v).to(dtype)
        loss = t if loss is None else loss + t
        mag += abs(float(t))
    return loss, mag


def loss_fold_bound(mag: float, ntaps: int):
    return (2 * ntaps + 1) * U * mag


# ---------------------------------------------------------------------------------------------- whole loss
def build_features(widths=NARROW, seed: int = 0) -> nn.Sequential:
    """Conv2d(3x3, padding 1) -> ReLU per width, MaxPool2d(2, 2) per "M"; He-normal weights and biases uniform in
    +-0.1 from ``seed`` (both ReLU branches populated)."""
    g = torch.Generator().manual_seed(seed)
    mods, cin = [], 3
    for w in widths:
        if w == "M":
            mods.append(nn.MaxPool2d(2, 2))
            continue
        conv = nn.Conv2d(cin, w, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
            conv.bias.copy_(torch.rand(w, generator=g) * 0.2 - 0.1)
        mods += [conv, nn.ReLU()]
        cin = w
    return nn.Sequential(*mods)


def make_images(N: int, C: int, H: int, W: int, seed: int):
    """target uniform in [0, 1], recon = clamp(target + 0.25 noise, 0, 1): |r - t| is not small."""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(N, C, H, W, generator=g)
    recon = (target + 0.25 * torch.randn(N, C, H, W, generator=g)).clamp(0, 1)
    return recon, target


def perc_oracle(features, recon, target, resize=None, layers=(3, 8, 15, 22), weights=(1.0, 1.0, 1.0, 1.0),
                dtype=F32):
    """(loss, [tap values]) of the perceptual loss on the CPU in ``dtype``, differentiable to ``recon``: a 1-channel
    image repeated to 3, optional bilinear resize (align_corners=False), no normalisation, then
    sum_l w_l mean |f_l(rec) - f_l(target)| over the outputs of ``layers``; the weights follow the layers in
    ascending order and a shorter list is filled with 1.0."""
    N = recon.shape[0]
    x = torch.cat([recon.to(dtype), target.to(dtype)])
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    if resize is not None:
        size = (resize, resize) if isinstance(resize, int) else tuple(resize)
        x = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    taps = sorted(set(int(v) for v in layers))
    wi = iter(weights)
    loss, values = None, []
    for i, m in enumerate(features):
        if isinstance(m, nn.Conv2d):
            x = F.conv2d(x, m.weight.detach().to(dtype), m.bias.detach().to(dtype), padding=1)
        elif isinstance(m, nn.ReLU):
            x = F.relu(x)
        else:
            x = F.max_pool2d(x, 2, 2)
        if i in taps:
            v = (x[:N] - x[N:]).abs().mean()
            term = float(next(wi, 1.0)) * v
            loss = term if loss is None else loss + term
            values.append(v)
        if i >= taps[-1]:
            break
    return loss, values
