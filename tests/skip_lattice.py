"""The ResBlock backward's skip pass and dropout ("Skip pass and dropout: exact lattice"): the
fp64 statement of fmd_conv_gn_apply (csrc/conv.hip, instances IG_GNA64 / IG_GNA128), fmd_skip_bwd (csrc/skip_bwd.hip)
and fmd_dropout_apply (csrc/groupnorm.hip) as operations of their own, the lattice on which they are exact, the cases,
the shared checks, and an fp32 emulation with mutants.  TEST INFRASTRUCTURE ONLY; imports without a GPU.

Layout (that of misc_ref.py): ``check_*(O, dev, ...)`` is the whole test of one case against an ``ops``-like namespace.
test_gpu_skip_lattice.py passes ``fmdiff.runtime.ops`` and "cuda"; test_skip_lattice.py passes ``Emu()`` and "cpu", so
every check is proved on the CPU first, and ``Emu(mutant=...)`` shows that the same check at the same shapes rejects
a kernel that is wrong in a known way.  No expected value comes from another kernel.

The skip pass, in fp64 (dy [M][Kd], W [Kd][C], dz / x / dx [M][C] split over two sources at C0, P / Q / R [N][C]):
    conv[p][c] = sum_k dy[p][k] W[k][c]
    dx[p][c]   = RNE_bf16( RNE_bf16(conv) + P[n][c] dz[p][c] + Q[n][c] x[p][c] + R[n][c] (+ old dx[p][c]) ), n = p // HW
    dW[k][c]   = sum_p dy[p][k] x[p][c]  (+ old dW)
    db[k]      = sum_p dy[p][k]          (+ old db)
The inner rounding of the conv term is part of the contract: both kernels pass it through LDS as bf16 (pack2).

Lattice: dy = k/4 |k| <= 12, W = k/8 |k| <= 8, dz, x = k/4 |k| <= 8, P in {-1, -1/2, 1/2, 1, 2}, Q = k/4 |k| <= 4,
R = k/4 |k| <= 8, old dx = k/4 |k| <= 16, old dW / db = k/4 |k| <= 64.  With Kd <= 256 every product and partial sum
of dx is a multiple of 1/32 below 2^11; with M <= 512 those of dW / db are multiples of 1/16 below 2^12: exact in
fp32 in any order, under any split, with or without FMA contraction (``conditions`` asserts this from the tensors).
dx must therefore be bit-equal to the reference, dW / db equal to the fp64 value outright.

Dropout: keep = mix32(key ^ index) >= p 2^32 with key = mix32(seed 0x9e3779b9 + salt) and the flat NHWC element
index (oracle/dropout.py); y = x keep / (1 - p); with ep = (h, a, b): y = dy keep / (1 - p) silu'(a[n][c] h + b[n][c]).
x = k/4, 1 <= |k| <= 31 (never 0, so the zeros of y ARE the mask) and p in {0, 1/2, 3/4} (scale 1, 2, 4) is exact.
Bounds (u = 2^-24, U = 2^-8, asserted with attn_bounds.check at MARGIN):
    p = 0.3 forward   scale = fl(1 / fl(1 - p)) (2u), the product (u), the bf16 store (U): (U + 3u) |ref| with
                      ref = x keep / (1 - f32(p))
    backward          z = fl(fl(a h) + b) or one fma: |dz| <= 2u (|a h| + |b|), carried by |silu''| <= 1/2;
                      g = silu'(z) evaluated with e_silu_grad(z) (misc_ref.py); scale, m = scale g and dy m round 3
                      times: U |ref| + |dy| scale (e_silu_grad(z) + u (|a h| + |b|)) + 3u |ref|

Largest err / bound seen on an MI355X (check()'s return value; every other check here is bit equality):
    dropout fwd p=0.3   0.835 (840 and 1680 elements: one bf16 rounding against a bound of one)
    dropout bwd         0.993 (p = 1/2; 0.974 at p = 0.3): one bf16 rounding again, met, not padded
The fp32 emulation on the CPU gives the same figures: 0.835 and 0.993 (0.974 at p = 0.3).
"""
from __future__ import annotations

import functools
import math
import types
import zlib

import numpy as np
import torch

from conv_lattice import bf16_rne
from misc_ref import (BF16, F32, F64, MARGIN, TINY, U, assert_equal, assert_guards, check,  # noqa: F401
                      e_silu_grad, guarded, lat, note, rng, silu_grad64)
from gn_bounds import U32

NAN = float("nan")
P_SET = (-1.0, -0.5, 0.5, 1.0, 2.0)
ACCS = ((0, 0), (1, 0), (0, 1), (1, 1))
MIN_SHARE = 0.01      # of dx elements: conv term changed by its rounding, double rounding visible, exact ties


# ================================================================================================ the skip pass
def case(name, inst, N, sp, C0, C1, Kd, seed=1):
    c = types.SimpleNamespace(name=name, inst=inst, N=N, sp=tuple(sp), C0=C0, C1=C1, Kd=Kd, seed=seed)
    c.C = C0 + C1
    c.HW = math.prod(sp)
    c.M = N * c.HW
    return c


# fmd_conv_gn_apply.  C: the block input's channels (the conv's output), Kd: those of dy.  The library does not
# report the instance; fmd_conv_gn_apply takes IG_GNA64 (64-channel tiles) up to C = 64 and IG_GNA128 above, both on
# 128-pixel tiles with a 32-wide K step (``gna_tile``).
GNA_CASES = [
    # Kd no multiple of the K step; the seam inside the tile on an 8-channel chunk; one partial tile over 3 images
    case("gna64_k24_seam40", "IG_GNA64", 3, (5, 7), 40, 24, 24),
    # single source (x1 / dx1 NULL); M = 180: the second tile is partial
    case("gna64_k256_single", "IG_GNA64", 3, (6, 10), 64, 0, 256),
    # C = 136: the second channel tile holds 8 channels, the seam is off the tile boundary; M = 189
    case("gna128_k72_c136", "IG_GNA128", 3, (7, 9), 72, 64, 72),
    # M = 288: the third tile straddles the images
    case("gna128_k128_c384", "IG_GNA128", 2, (12, 12), 256, 128, 128),
    # a volume: the wrapper's (D H, W) plane
    case("gna128_k128_vol", "IG_GNA128", 2, (2, 5, 7), 128, 0, 128),
    # the geometry of gna128_k72_c136 at the Kd fmd_skip_bwd takes (its third Kd = 128 geometry)
    case("gna128_k128_c136", "IG_GNA128", 3, (7, 9), 72, 64, 128),
]
# fmd_skip_bwd (Kd = 128, C > 64; 64-pixel tiles, 128-channel c-tiles).  Tiles: 5 / 3 / 3 / 2 / 8, the last partial.
SKIP_CASES = [
    case("skip_c384_m288", "skip_bwd", 2, (12, 12), 256, 128, 128),
    case("skip_vol_m140", "skip_bwd", 2, (2, 5, 7), 128, 0, 128),
    case("skip_c136_m189", "skip_bwd", 3, (7, 9), 72, 64, 128),
    case("skip_c136_m105", "skip_bwd", 3, (5, 7), 72, 64, 128),
    # 8 tiles: groups = 8 owns one tile each, groups = 16 leaves 8 idle, groups = 3 is uneven
    case("skip_c256_m480", "skip_bwd", 2, (15, 16), 128, 128, 128),
]
SKIP_GROUPS = (1, 3, 8, 16)     # forced pixel groups; 8, 16: the G % 8 == 0 block map
# (acc0, acc1) of a forced-groups run with accumulate=True; accumulate=False runs the complement
SKIP_ACC = {1: (1, 1), 3: (0, 1), 8: (1, 0), 16: (0, 0)}
BY_NAME = {c.name: c for c in GNA_CASES + SKIP_CASES}
assert len(BY_NAME) == len(GNA_CASES) + len(SKIP_CASES)


def gna_tile(c):
    """(channels, pixels) of the tile fmd_conv_gn_apply runs case ``c`` on."""
    return (64 if c.C <= 64 else 128), 128


def accs(c):
    return ACCS if c.C1 else ((0, 0), (1, 0))


def _nz_lat(shape, g, kmax, den, dtype=F32):
    """k / den with 1 <= |k| <= kmax."""
    k = torch.randint(1, kmax + 1, tuple(shape), generator=g)
    s = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    return ((k * s).double() / den).to(dtype)


@functools.lru_cache(maxsize=None)
def generate(name):
    """The seeded CPU operands of case ``name``: bf16 activations, fp32 weight master [Kd][C][1][1] and vectors."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + c.seed)
    N, sp, C0, C1, C, Kd = c.N, c.sp, c.C0, c.C1, c.C, c.Kd
    T = dict(dy=lat((N, *sp, Kd), g, 12, 4, BF16), w=lat((Kd, C, 1, 1), g, 8, 8), dz=lat((N, *sp, C), g, 8, 4, BF16),
             x=lat((N, *sp, C), g, 8, 4, BF16), Q=lat((N, C), g, 4, 4), R=lat((N, C), g, 8, 4),
             old=lat((N, *sp, C), g, 16, 4, BF16), dw0=lat((Kd, C, 1, 1), g, 64, 4), db0=lat((Kd,), g, 64, 4))
    T["P"] = torch.tensor(P_SET)[torch.randint(0, len(P_SET), (N, C), generator=g)]
    return T


@functools.lru_cache(maxsize=None)
def reference(name, acc0=0, acc1=0, accumulate=False):
    """The operation statement of the module docstring in fp64.  dx [M][C] is the rounded result; ``conv`` the
    unrounded conv term, ``conv_r`` the rounded one, ``s`` the sum the final rounding sees, ``single`` what one
    rounding of the unrounded sum would give."""
    c, T = BY_NAME[name], generate(name)
    M, C, C0 = c.M, c.C, c.C0
    dy, x = T["dy"].double().reshape(M, -1), T["x"].double().reshape(M, C)
    conv = dy @ T["w"].double().reshape(c.Kd, C)
    n = torch.arange(M) // c.HW
    rest = T["P"].double()[n] * T["dz"].double().reshape(M, C) + T["Q"].double()[n] * x + T["R"].double()[n]
    accm = torch.cat([torch.full((C0,), float(acc0)), torch.full((C - C0,), float(acc1))]).double()
    rest = rest + T["old"].double().reshape(M, C) * accm
    conv_r = bf16_rne(conv)
    s = conv_r + rest
    dw, db = dy.t() @ x, dy.sum(0)
    if accumulate:
        dw, db = dw + T["dw0"].double().reshape(c.Kd, C), db + T["db0"].double()
    return dict(conv=conv, conv_r=conv_r, s=s, dx=bf16_rne(s), single=bf16_rne(conv + rest), dw=dw, db=db)


def _on(t, den, kmax, what):
    q = t.double() * den
    assert torch.equal(q, q.round()) and float(q.abs().max()) <= kmax, f"{what} leaves its lattice"


@functools.lru_cache(maxsize=None)
def conditions(name):
    """Assert what the exactness argument needs of case ``name`` from its actual tensors, and that the case is not
    vacuous: for every (acc0, acc1) it runs with, at least MIN_SHARE of the dx elements have a conv term its bf16
    rounding changes, differ between the double-rounded statement and a single rounding, and are round-to-even ties
    of the final rounding.  Returns {(acc0, acc1): (conv share, double-rounding share, tie share)}."""
    c, T = BY_NAME[name], generate(name)
    M, C, Kd = c.M, c.C, c.Kd
    assert Kd <= 256 and M <= 512 and c.C0 % 8 == 0 and c.C1 % 8 == 0
    for k, den, kmax in (("dy", 4, 12), ("w", 8, 8), ("dz", 4, 8), ("x", 4, 8), ("Q", 4, 4), ("R", 4, 8),
                         ("old", 4, 16), ("dw0", 4, 64), ("db0", 4, 64)):
        _on(T[k], den, kmax, f"{name}: {k}")
    assert all(v in P_SET for v in T["P"].unique().tolist())
    for k in ("dy", "w", "dz", "x", "old"):       # MFMA / bf16 operands survive a bf16 round trip
        assert torch.equal(T[k].double(), T[k].to(BF16).double()), f"{name}: {k} is not a bf16 value"
    # the caps: with |operands| every partial sum, in any order and under any split, is bounded by the same sum
    dy, x = T["dy"].double().abs().reshape(M, Kd), T["x"].double().abs().reshape(M, C)
    n = torch.arange(M) // c.HW
    aconv = dy @ T["w"].double().abs().reshape(Kd, C)
    adx = (aconv * (1 + U) + T["P"].double().abs()[n] * T["dz"].double().abs().reshape(M, C)
           + T["Q"].double().abs()[n] * x + T["R"].double().abs()[n] + T["old"].double().abs().reshape(M, C))
    assert float(adx.max()) < 2.0 ** 11, f"{name}: a dx partial sum can reach {float(adx.max())}"
    adw = dy.t() @ x + T["dw0"].double().abs().reshape(Kd, C)
    adb = dy.sum(0) + T["db0"].double().abs()
    assert float(adw.max()) < 2.0 ** 12 and float(adb.max()) < 2.0 ** 12, f"{name}: a dW / db partial sum too large"
    out = {}
    for a0, a1 in accs(c):
        R = reference(name, a0, a1, True)
        for k, step in (("conv", 32), ("s", 32), ("dw", 16), ("db", 4)):     # 2^11 * 32, 2^12 * 16 < 2^24
            q = R[k] * step
            assert torch.equal(q, q.round()), f"{name}: {k} leaves the 1/{step} lattice"
        assert torch.equal(R["s"].float().double(), R["s"])
        low = R["s"].float().contiguous().view(torch.int32) & 0xFFFF
        sh = (float((R["conv_r"] != R["conv"]).double().mean()), float((R["single"] != R["dx"]).double().mean()),
              float((low == 0x8000).double().mean()))
        assert min(sh) >= MIN_SHARE, f"{name} acc {a0}{a1}: conv / double rounding / tie shares {sh} below 1 %"
        assert bool((R["dw"].abs().sum(1) > 0).all()) and bool((R["db"] != 0).any())
        out[(a0, a1)] = sh
    return out


def _operands(c, dev, acc0, acc1):
    """Device operands of one launch: inputs, and guarded outputs -- an accumulated destination holds the old dx, an
    overwritten one NaN (reading it would poison the result); dx1 does not exist where C1 = 0."""
    T = generate(c.name)
    C0 = c.C0
    a = types.SimpleNamespace()
    a.dy, a.dz = T["dy"].to(dev), T["dz"].to(dev)
    a.x0 = T["x"][..., :C0].contiguous().to(dev)
    a.x1 = T["x"][..., C0:].contiguous().to(dev) if c.C1 else None
    a.P, a.Q, a.R = T["P"].to(dev), T["Q"].to(dev), T["R"].to(dev)
    a.b0, a.dx0 = guarded((c.N, *c.sp, C0), BF16, dev, T["old"][..., :C0] if acc0 else NAN)
    a.b1, a.dx1 = guarded((c.N, *c.sp, c.C1), BF16, dev, T["old"][..., C0:] if acc1 else NAN) if c.C1 else (None, None)
    return a, T


def _assert_dx(c, a, R, name):
    assert_guards(a.b0, f"{name} dx0")
    dx = R["dx"].reshape(c.N, *c.sp, c.C)
    assert_equal(a.dx0, dx[..., :c.C0], f"{name} dx0", bf16=True)
    if c.C1:
        assert_guards(a.b1, f"{name} dx1")
        assert_equal(a.dx1, dx[..., c.C0:], f"{name} dx1", bf16=True)


def check_gn_apply(O, dev, name, acc0, acc1):
    """fmd_conv_gn_apply on case ``name``: dx bit-equal to the fp64 statement, nothing written outside dx."""
    c = BY_NAME[name]
    conditions(name)
    assert c.inst == ("IG_GNA64" if gna_tile(c)[0] == 64 else "IG_GNA128")
    a, T = _operands(c, dev, acc0, acc1)
    wt = O.prep_weights(T["w"].to(dev), 1)
    assert tuple(wt.shape) == (c.C, 1, c.Kd) and wt.dtype == BF16
    O.conv1x1_gn_apply(a.dy, wt, a.dz, a.x0, a.x1, a.P, a.Q, a.R, a.dx0, acc0, a.dx1, acc1)
    _assert_dx(c, a, reference(name, acc0, acc1), f"{name} acc {acc0}{acc1}")


def check_skip_bwd(O, dev, name, groups, accumulate):
    """fmd_skip_bwd on case ``name`` with ``groups`` forced pixel groups (0: the plan's own count): the plan's
    slabs and workgroups, dx bit-equal, dW and db equal to the fp64 value outright."""
    c = BY_NAME[name]
    conditions(name)
    acc0, acc1 = SKIP_ACC.get(groups, (1, 0))
    if not accumulate:
        acc0, acc1 = 1 - acc0, 1 - acc1
    if not c.C1:
        acc1 = 0
    tag = f"{name} groups {groups} accumulate {accumulate} acc {acc0}{acc1}"
    tiles, ntc = -(-c.M // 64), -(-c.C // 128)
    plan = O.skip_bwd_plan(c.N, c.HW, c.C0, c.C1, c.Kd, groups, min_tiles=0)
    assert plan is not None and plan.c_tile == 128, f"{tag}: the plan refuses"
    if groups:
        assert plan.slabs == min(groups, tiles), f"{tag}: {plan.slabs} slabs"
        assert plan.workgroups == groups * ntc, f"{tag}: {plan.workgroups} workgroups"
    else:
        assert 1 <= plan.slabs <= tiles and plan.workgroups % ntc == 0
    assert plan.ws_floats == plan.slabs * (c.Kd * c.C + c.Kd)
    a, T = _operands(c, dev, acc0, acc1)
    bw, dw = guarded((c.Kd, c.C, 1, 1), F32, dev, T["dw0"] if accumulate else NAN)
    bb, db = guarded((c.Kd,), F32, dev, T["db0"] if accumulate else NAN)
    wt = O.prep_weights(T["w"].to(dev), 1)
    taken = O.skip_bwd(a.dy, wt, a.dz, a.x0, a.x1, a.P, a.Q, a.R, a.dx0, acc0, a.dx1, acc1, dw, db,
                       accumulate=accumulate, groups=groups, min_tiles=0)
    assert taken, f"{tag}: not taken"
    R = reference(name, acc0, acc1, accumulate)
    _assert_dx(c, a, R, tag)
    assert_guards(bw, f"{tag} dW")
    assert_guards(bb, f"{tag} db")
    assert_equal(dw.reshape(c.Kd, c.C), R["dw"], f"{tag} dW")
    assert_equal(db, R["db"], f"{tag} db")


# ================================================================================================ dropout
DROP_SHAPES = {
    "hw35_c24": (3, (5, 7), 24),          # the index is no power of two; HW = 35 with three images
    "vol_c8": (2, (3, 5, 7), 8),
    # 2 097 432 eight-channel units against the grid cap of 8192 blocks of 256: the grid-stride loop's second trip
    "stride_c64": (1, (262179, 1), 64),
}
DROP_P = (0.0, 0.5, 0.75, 0.3)
DROP_SEEDS = (5, 123456789)               # seed 0x9e3779b9 wraps 2^32 for both
DROP_SALTS = (3, 0x9E3779B1)              # the second is >= 2^31
BWD_SHAPE = "hw35_c24"
BWD_P = (0.5, 0.3)


def keep_ref(seed, salt, shape, p):
    from oracle.dropout import keep_mask_nhwc
    return torch.from_numpy(keep_mask_nhwc(seed, salt, shape, p))


def drop_scale(p):
    """1 / (1 - p) with p at its fp32 ABI value, in fp64."""
    return 1.0 / (1.0 - float(torch.tensor(p, dtype=F32)))


def _seed(seed, dev):
    return torch.tensor([seed], dtype=torch.int32).to(dev)


def _fwd_once(O, dev, x, p, seed, salt, inplace, tag):
    """One forward launch in guarded buffers; returns y on the CPU.  In place: x's own buffer is the output."""
    if inplace:
        buf, xd = guarded(tuple(x.shape), BF16, dev, x)
        y = O.dropout_apply(xd, p, _seed(seed, dev), salt, out=xd)
        assert y.data_ptr() == xd.data_ptr(), f"{tag}: out= not reused"
    else:
        xd = x.to(dev)
        buf, out = guarded(tuple(x.shape), BF16, dev, NAN)
        y = O.dropout_apply(xd, p, _seed(seed, dev), salt, out=out)
        assert torch.equal(xd.cpu(), x), f"{tag}: x modified by an out-of-place call"
    assert_guards(buf, tag)
    return y.cpu()


def _assert_fwd(y, x, keep, p, tag):
    assert torch.equal(y == 0, ~keep), f"{tag}: {int(((y == 0) != ~keep).sum())} mask elements differ from the oracle's"
    ref = x.double() * keep.double() * drop_scale(p)
    if p in (0.0, 0.5, 0.75):
        assert_equal(y, ref, tag, bf16=True)
        if p == 0.0:
            assert torch.equal(y, x), f"{tag}: p = 0 must return x bit for bit"
        return None
    return note("dropout fwd p=0.3", check(y, ref, (U + 3 * U32) * ref.abs(), tag))


def check_dropout_fwd(O, dev, shape, p):
    """Forward of one (shape, p): every (seed, salt) pair, out of place twice and in place, against the oracle's mask
    and x keep / (1 - p); distinct pairs give distinct masks.  The grid-stride shape runs one pair, out of place."""
    N, sp, C = DROP_SHAPES[shape]
    sh = (N, *sp, C)
    x = _nz_lat(sh, rng(71), 31, 4, BF16)
    big = shape == "stride_c64"
    pairs = [(DROP_SEEDS[1], DROP_SALTS[1])] if big else [(s, t) for s in DROP_SEEDS for t in DROP_SALTS]
    masks, r = [], None
    for seed, salt in pairs:
        tag = f"dropout {shape} p={p} seed={seed} salt={salt:#x}"
        keep = keep_ref(seed, salt, sh, p)
        y = _fwd_once(O, dev, x, p, seed, salt, False, tag)
        r = _assert_fwd(y, x, keep, p, tag) or r
        if not big:
            assert torch.equal(_fwd_once(O, dev, x, p, seed, salt, False, tag), y), f"{tag}: two calls differ"
            assert torch.equal(_fwd_once(O, dev, x, p, seed, salt, True, tag + " in place"), y), \
                f"{tag}: in place differs from out of place"
        masks.append(y == 0)
    if p > 0:
        rate = float(torch.stack(masks).double().mean())
        assert abs(rate - p) < 0.05, f"dropout {shape} p={p}: drop rate {rate}"
        for i in range(len(masks)):
            for j in range(i):
                assert not torch.equal(masks[i], masks[j]), \
                    f"dropout {shape} p={p}: pairs {pairs[i]}, {pairs[j]} share a mask"
    return r


def bwd_inputs(seed=73):
    N, sp, C = DROP_SHAPES[BWD_SHAPE]
    g = rng(seed)
    sh = (N, *sp, C)
    return dict(dy=_nz_lat(sh, g, 31, 4, BF16), h=torch.randn(sh, generator=g).to(BF16),
                a=torch.rand((N, C), generator=g) + 0.5, b=torch.randn((N, C), generator=g) * 0.2)


def bwd_ref(d, keep, p):
    """(ref, bound) of the backward in fp64 (module docstring)."""
    N, C = d["a"].shape
    a, b = (v.double().reshape(N, *[1] * (d["h"].dim() - 2), C) for v in (d["a"], d["b"]))
    h, dy = d["h"].double(), d["dy"].double()
    z = a * h + b
    sc = drop_scale(p)
    ref = dy * keep.double() * sc * silu_grad64(z)
    bnd = U * ref.abs() + dy.abs() * keep.double() * sc * (e_silu_grad(z) + U32 * ((a * h).abs() + b.abs())) \
        + 3 * U32 * ref.abs()
    return ref, bnd


def check_dropout_bwd(O, dev, p):
    """ep = (h, a, b) on N = 3, HW = 35, out of place and in place: the bound, and zeros that are exactly the
    forward's for the same (seed, salt)."""
    d = bwd_inputs()
    sh = tuple(d["dy"].shape)
    r = 0.0
    for seed, salt in ((DROP_SEEDS[0], DROP_SALTS[1]), (DROP_SEEDS[1], DROP_SALTS[0])):
        tag = f"dropout bwd p={p} seed={seed} salt={salt:#x}"
        keep = keep_ref(seed, salt, sh, p)
        fwd = _fwd_once(O, dev, d["dy"], p, seed, salt, False, tag + " (forward)")
        buf, out = guarded(sh, BF16, dev, NAN)
        # a, b of an image past the last must never be read
        ab = [torch.cat([v, torch.full_like(v[:1], NAN)]).to(dev)[:v.shape[0]] for v in (d["a"], d["b"])]
        y = O.dropout_apply(d["dy"].to(dev), p, _seed(seed, dev), salt, ep=(d["h"].to(dev), *ab), out=out).cpu()
        assert_guards(buf, tag)
        bi, dyi = guarded(sh, BF16, dev, d["dy"])          # in place, as the engine calls it
        yi = O.dropout_apply(dyi, p, _seed(seed, dev), salt, ep=(d["h"].to(dev), *ab), out=dyi)
        assert_guards(bi, tag + " in place")
        assert yi.data_ptr() == dyi.data_ptr() and torch.equal(yi.cpu(), y), f"{tag}: in place differs"
        assert torch.equal(y == 0, fwd == 0), f"{tag}: the backward's zeros are not the forward's"
        assert torch.equal(y == 0, ~keep), f"{tag}: mask differs from the oracle's"
        ref, bnd = bwd_ref(d, keep, p)
        r = max(r, note(f"dropout bwd p={p}", check(y, ref, bnd, tag)))
    return r


# ================================================================================================ case registry
def _cases():
    out = {"gn_apply": {}, "skip_bwd": {}, "dropout_fwd": {}, "dropout_bwd": {}}
    for c in GNA_CASES:
        for a0, a1 in accs(c):
            out["gn_apply"][f"{c.name}-acc{a0}{a1}"] = functools.partial(check_gn_apply, name=c.name, acc0=a0, acc1=a1)
    for c in SKIP_CASES:
        for g in (0,) + SKIP_GROUPS:
            for acc in ((True,) if g == 0 else (True, False)):
                out["skip_bwd"][f"{c.name}-g{g}-{'acc' if acc else 'ovw'}"] = functools.partial(
                    check_skip_bwd, name=c.name, groups=g, accumulate=acc)
    for s in DROP_SHAPES:
        for p in ((0.5,) if s == "stride_c64" else DROP_P):
            out["dropout_fwd"][f"{s}-p{p}"] = functools.partial(check_dropout_fwd, shape=s, p=p)
    for p in BWD_P:
        out["dropout_bwd"][f"p{p}"] = functools.partial(check_dropout_bwd, p=p)
    return out


CASES = _cases()


def case_ids(families=None):
    return [(f, c) for f in (families or CASES) for c in CASES[f]]


def _skip_id(cid):
    """(case, groups) of a skip_bwd / gn_apply case id."""
    name, *rest = cid.split("-")
    return BY_NAME[name], (int(rest[0][1:]) if rest and rest[0].startswith("g") else None)


def _straddles(c, bpx):
    """Some pixel's image differs from that of its tile's first pixel."""
    p = torch.arange(c.M)
    return bool(((p // c.HW) != ((p // bpx * bpx) // c.HW)).any())


def _bpx(family):
    return 128 if family == "gn_apply" else 64


def _bco(family, cid):
    return gna_tile(_skip_id(cid)[0])[0] if family == "gn_apply" else 128


def _has_acc(family, cid, both=False):
    c, g = _skip_id(cid)
    if family == "gn_apply":
        a0, a1 = int(cid[-2]), int(cid[-1])
    else:
        a0, a1 = SKIP_ACC.get(g, (1, 0))
        if cid.endswith("ovw"):
            a0, a1 = 1 - a0, 1 - a1
        if not c.C1:
            a1 = 0
    return (a0 != a1 and c.C1 > 0) if both else bool(a0 or a1)


# mutant -> (what it does, families, applies(family, case id): the cases in which the bug can show at all)
DX = ("gn_apply", "skip_bwd")
MUTANTS = {
    "conv_not_rounded": ("conv term not rounded to bf16", DX, lambda f, c: True),
    "store_truncated": ("final store truncated", DX, lambda f, c: True),
    "store_half_away": ("final store rounded half away from zero", DX, lambda f, c: True),
    "n_from_tile_start": ("n taken from the tile's first pixel", DX,
                          lambda f, c: _straddles(_skip_id(c)[0], _bpx(f))),
    "source_per_tile": ("source chosen per channel tile instead of per 8-channel chunk", DX,
                        lambda f, c: _skip_id(c)[0].C0 % _bco(f, c) != 0),
    "acc_swapped": ("acc0 / acc1 swapped", DX, lambda f, c: _has_acc(f, c, both=True)),
    "old_ignored": ("old dx ignored", DX, lambda f, c: _has_acc(f, c)),
    "r_image0": ("R of image 0 for every image", DX, lambda f, c: True),
    "last_tile_dropped": ("last partial pixel tile dropped from dW", ("skip_bwd",),
                          lambda f, c: _skip_id(c)[0].M % 64 != 0),
    "stale_slab": ("an idle group's stale slab added", ("skip_bwd",),
                   lambda f, c: (_skip_id(c)[1] or 0) > -(-_skip_id(c)[0].M // 64)),
    "db_per_ctile": ("db summed once per channel tile", ("skip_bwd",), lambda f, c: _skip_id(c)[0].C > 128),
    "old_dw_dropped": ("old dW dropped under accumulate", ("skip_bwd",), lambda f, c: c.endswith("acc")),
    "idx_no_channel": ("element index without the channel term", ("dropout_fwd", "dropout_bwd"),
                       lambda f, c: "c8" not in c and "p0.0" not in c),
    "idx_nchw": ("index in NCHW order", ("dropout_fwd", "dropout_bwd"), lambda f, c: "p0.0" not in c),
    "seed_plus_1": ("seed + 1", ("dropout_fwd", "dropout_bwd"), lambda f, c: "p0.0" not in c),
    "salt_ignored": ("salt ignored", ("dropout_fwd", "dropout_bwd"), lambda f, c: "p0.0" not in c),
    "scale_omitted": ("scale omitted", ("dropout_fwd", "dropout_bwd"), lambda f, c: "p0.0" not in c),
    "p_for_1mp": ("p in place of 1 - p in the scale", ("dropout_fwd", "dropout_bwd"), lambda f, c: "p0.5" not in c),
    "ab_image0": ("a / b of image 0 for every image", ("dropout_bwd",), lambda f, c: True),
    "bwd_mask_shift8": ("backward mask drawn with the forward's index shifted by 8", ("dropout_bwd",),
                        lambda f, c: True),
    "silu_not_grad": ("SiLU in place of SiLU'", ("dropout_bwd",), lambda f, c: True),
}
# the mutants aimed at the edge each skip-pass case exists for: at least one must reject it (every acc / groups run)
EDGE = {
    "gna64_k24_seam40": ("source_per_tile", "n_from_tile_start"),
    "gna64_k256_single": ("n_from_tile_start", "conv_not_rounded"),
    "gna128_k72_c136": ("source_per_tile",),
    "gna128_k128_c384": ("n_from_tile_start", "acc_swapped"),
    "gna128_k128_vol": ("n_from_tile_start", "r_image0"),
    "gna128_k128_c136": ("source_per_tile",),
    "skip_c384_m288": ("last_tile_dropped", "db_per_ctile", "stale_slab"),
    "skip_vol_m140": ("last_tile_dropped", "stale_slab"),
    "skip_c136_m189": ("last_tile_dropped", "source_per_tile"),
    "skip_c136_m105": ("last_tile_dropped", "stale_slab"),
    "skip_c256_m480": ("last_tile_dropped", "stale_slab", "db_per_ctile"),
}


def mutant_cases(mutant):
    _, fams, applies = MUTANTS[mutant]
    return [(f, c) for f in fams for c in CASES[f] if applies(f, c)]


# ================================================================================================ fp32 emulation
def _trunc_bf16(v):
    return (v.float().contiguous().view(torch.int32) & ~0xFFFF).view(F32).to(BF16)


def _half_away_bf16(v):
    """fp32 -> bf16, ties away from zero (add half a bf16 ulp to the magnitude, then drop the low bits)."""
    return ((v.float().contiguous().view(torch.int32) + 0x8000) & ~0xFFFF).view(F32).to(BF16)


def _silu_grad32(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


class Emu:
    """fp32 CPU emulation of the documented arithmetic behind the wrappers' signatures.  The conv term accumulates
    over explicit 32-wide K steps, dW / db over explicit 64-pixel tiles into one fp32 slab per pixel group, the slabs
    are then summed in slab order; ``perm=True`` walks the K steps, the tiles, the slabs and the epilogue's terms in
    reverse, which must not change one bit on the lattice.  ``mutant``: a key of MUTANTS."""

    def __init__(self, mutant=None, perm=False):
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.perm = mutant, perm

    def _ord(self, it):
        it = list(it)
        return it[::-1] if self.perm else it

    # ---------------------------------------------------------------------------------------------- skip pass
    @staticmethod
    def prep_weights(w, mode):
        assert mode == 1 and w.shape[2:] == (1, 1)
        Kd, C = w.shape[:2]
        return w.reshape(Kd, C).t().contiguous().to(BF16).reshape(C, 1, Kd)

    def _dx(self, dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1, acc1, bpx, bco):
        mu = self.mutant
        N, Kd, C, C0 = dy.shape[0], dy.shape[-1], dz.shape[-1], x0.shape[-1]
        M = dy.numel() // Kd
        HW = M // N
        dyf, W = dy.reshape(M, Kd).float(), wgt_t.reshape(C, Kd).float()
        conv = torch.zeros(M, C)
        for k0 in self._ord(range(0, Kd, 32)):
            conv = conv + dyf[:, k0:k0 + 32] @ W[:, k0:k0 + 32].t()
        ve = conv if mu == "conv_not_rounded" else conv.to(BF16).float()
        p, ch = torch.arange(M), torch.arange(C)
        n = (p // bpx * bpx) // HW if mu == "n_from_tile_start" else p // HW
        nR = torch.zeros_like(n) if mu == "r_image0" else n
        first = (ch // bco * bco < C0) if mu == "source_per_tile" else (ch // 8 * 8 < C0)

        def gather(s0, s1):
            """[M][C] as the pointer arithmetic reads the two sources (a wrong ``first`` runs into the next pixel)."""
            f0 = s0.reshape(-1).float()
            v = f0[(p[:, None] * C0 + ch[None, :]).clamp(max=f0.numel() - 1)]
            if s1 is None:
                return v
            f1, C1 = s1.reshape(-1).float(), C - C0
            return torch.where(first[None, :], v, f1[(p[:, None] * C1 + ch[None, :] - C0).clamp(0, f1.numel() - 1)])
        a0, a1 = (acc1, acc0) if mu == "acc_swapped" else (acc0, acc1)
        if mu == "old_ignored":
            a0 = a1 = 0
        accf = torch.where(first, torch.tensor(bool(a0)), torch.tensor(bool(a1)))
        x = gather(x0, x1)
        old = torch.where(accf[None, :], gather(dx0, dx1), torch.zeros(()))
        terms = [P[n] * dz.reshape(M, C).float(), Q[n] * x, R[nR], ve, old]
        s = torch.zeros(M, C)
        for t in self._ord(terms):
            s = s + t
        store = {"store_truncated": _trunc_bf16, "store_half_away": _half_away_bf16}.get(mu, lambda v: v.to(BF16))
        out = store(s)
        dx0.copy_(out[:, :C0].reshape(dx0.shape))
        if dx1 is not None:
            dx1.copy_(out[:, C0:].reshape(dx1.shape))

    def conv1x1_gn_apply(self, dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1=None, acc1=0):
        C = dz.shape[-1]
        self._dx(dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1, acc1, 128, 64 if C <= 64 else 128)

    @staticmethod
    def skip_bwd_plan(N, HW, C0, C1, Kd, groups=0, min_tiles=None, num_cu=256):
        """The documented plan (csrc/skip_bwd.hip ``decide``): forced groups as given, else two workgroups per CU
        over the c-tiles, at most one per tile, in whole multiples of 8."""
        C, M = C0 + C1, N * HW
        if Kd != 128 or C <= 64 or C0 % 8 or C1 % 8 or C0 < 8:
            return None
        ntp, ntc = -(-M // 64), -(-C // 128)
        G = groups
        if G <= 0:
            G = min(max(2 * num_cu // ntc, 1), ntp)
            G -= G % 8 if G >= 8 else 0
            if ntp < (min_tiles or 0) * G:
                return None
        nsl = min(G, ntp)
        return types.SimpleNamespace(taken=1, c_tile=128, workgroups=G * ntc, slabs=nsl, ws_floats=nsl * (Kd * C + Kd),
                                     G=G)

    def skip_bwd(self, dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1, acc1, dw, db, accumulate=True, groups=0,
                 min_tiles=None):
        mu = self.mutant
        N, Kd, C, C0 = dy.shape[0], dy.shape[-1], dz.shape[-1], x0.shape[-1]
        M = dy.numel() // Kd
        plan = self.skip_bwd_plan(N, M // N, C0, C - C0, Kd, groups, min_tiles)
        if plan is None:
            return False
        x = (x0 if x1 is None else torch.cat([x0, x1], -1)).reshape(M, C).float()
        dyf = dy.reshape(M, Kd).float()
        self._dx(dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1, acc1, 64, 128)
        G, ntp, ntc = plan.G, -(-M // 64), -(-C // 128)
        sw, sb = torch.zeros(plan.slabs, Kd, C), torch.zeros(plan.slabs, Kd)
        for grp in range(plan.slabs):
            for t in self._ord(range(grp, ntp, G)):
                sl = slice(64 * t, min(M, 64 * t + 64))
                if not (mu == "last_tile_dropped" and t == ntp - 1 and M % 64):
                    sw[grp] = sw[grp] + dyf[sl].t() @ x[sl]
                row = torch.zeros(Kd)
                for q in self._ord(range(sl.start, sl.stop)):
                    row = row + dyf[q]
                sb[grp] = sb[grp] + row
        keep_old = accumulate and mu != "old_dw_dropped"
        tw = dw.reshape(Kd, C).clone() if keep_old else torch.zeros(Kd, C)
        tb = db.clone() if accumulate else torch.zeros(Kd)
        for g in self._ord(range(plan.slabs)):
            tw, tb = tw + sw[g], tb + sb[g] * (ntc if mu == "db_per_ctile" else 1)
        if mu == "stale_slab" and G > ntp:                 # a slab no workgroup wrote, still summed
            tw, tb = tw + 0.25, tb + 0.25
        dw.copy_(tw.reshape(dw.shape))
        db.copy_(tb)
        return True

    # ---------------------------------------------------------------------------------------------- dropout
    def dropout_apply(self, x, p, seed, salt, ep=None, out=None):
        from oracle.dropout import M32, mix32
        mu = self.mutant
        N, C = x.shape[0], x.shape[-1]
        M = x.numel() // C
        HW = M // N
        sd = int(seed[0]) + (1 if mu == "seed_plus_1" else 0)
        st = 0 if mu == "salt_ignored" else int(salt) & 0xFFFFFFFF
        key = mix32(np.uint64((sd * 0x9E3779B9 + st) & 0xFFFFFFFF))
        pix = np.arange(M, dtype=np.uint64)[:, None]
        ch = np.arange(C, dtype=np.uint64)[None, :]

        def index(shift=0):
            if mu == "idx_nchw":
                return ((pix // np.uint64(HW)) * np.uint64(C) + ch) * np.uint64(HW) + pix % np.uint64(HW)
            c = ch % np.uint64(8) if mu == "idx_no_channel" else ch
            return (pix * np.uint64(C) + c + np.uint64(shift)) & M32
        p32 = float(torch.tensor(p, dtype=F32))
        thr = np.uint64(min(int(p32 * 4294967296.0), 4294967295))
        keep = torch.from_numpy(mix32(key ^ index(8 if (mu == "bwd_mask_shift8" and ep is not None) else 0)) >= thr)
        one = torch.ones((), dtype=F32)
        scale = one / (torch.tensor(p, dtype=F32) if mu == "p_for_1mp" else one - torch.tensor(p, dtype=F32))
        if mu == "scale_omitted":
            scale = one
        m = torch.where(keep, scale, torch.zeros(()))
        if ep is not None:
            h, a, b = ep
            n = torch.arange(M) // HW
            if mu == "ab_image0":
                n = torch.zeros_like(n)
            z = h.reshape(M, C).float() * a[n] + b[n]
            m = m * (z * torch.sigmoid(z) if mu == "silu_not_grad" else _silu_grad32(z))
        y = (x.reshape(M, C).float() * m).to(BF16).reshape(x.shape)
        if out is None:
            return y
        out.copy_(y)
        return out
